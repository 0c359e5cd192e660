/*
 * ragplan_check.cpp -- the row-class tables (csrc/at_classes.h) and the ragged planner (csrc/at_ragplan.h) without a GPU.
 * Built by `make asan` with AddressSanitizer and UBSan and run by tests/test_asan.py:
 *   1. every family's (g, k) for every read length 0 .. 1100 against the edge lists written out below;
 *   2. the planner's invariants over seeded length sets;
 *   3. eight plans against FNV-1a hashes recorded from the hand-written planning code that align_host carried before the planner
 *      was split out of it (its sorts, padding and bucket loops, with the launches recorded instead of issued).
 * Exit status 0 and "ragplan_check: ok" when everything holds; every failure is printed.
 */
#include "../../aligntools/c_amd/csrc/at_classes.h"
#include "../../aligntools/c_amd/csrc/at_ragplan.h"

#include <cstdio>
#include <cstring>

static int g_failures = 0;
#define CHECK(cond, ...)                                                        \
	do {                                                                        \
		if (!(cond)) {                                                          \
			if (++g_failures <= 40) { printf("FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
		}                                                                       \
	} while (0)

/* ---- 1. the class tables: edge lists as data ---- */
struct Edge { int max_l1, g, k; };
template <size_t N>
static Edge expect(const Edge (&e)[N], int l1)
{
	for (size_t q = 0; q < N; ++q) if (l1 <= e[q].max_l1) return e[q];
	return e[N - 1];   /* (longer reads never reach a table: the callers check the family's top first) */
}

static const Edge kU4[] = {{36, 4, 9}, {40, 4, 10}, {52, 4, 13}, {64, 4, 16}, {76, 4, 19}};
static const Edge kG8[] = {{40, 8, 5}, {48, 8, 6}, {56, 8, 7}, {64, 8, 8}, {80, 8, 10}, {104, 8, 13}, {128, 8, 16}, {152, 8, 19}};
static const Edge kG16[] = {{64, 16, 4}, {80, 16, 5}, {96, 16, 6}, {112, 16, 7}, {160, 16, 10}, {208, 16, 13}, {256, 16, 16}, {304, 16, 19}};
static const Edge kG32[] = {{224, 32, 7}, {256, 32, 8}, {320, 32, 10}, {384, 32, 12}, {416, 32, 13}, {512, 32, 16}, {608, 32, 19}};
static const Edge kG32Group32[] = {{224, 32, 7}, {256, 32, 8}, {320, 32, 10}, {416, 32, 13}, {512, 32, 16}, {608, 32, 19}};   /* AT_GROUP=32: no 12 rows */
static const Edge kG32Rag[] = {{320, 32, 10}, {384, 32, 12}, {416, 32, 13}, {512, 32, 16}, {608, 32, 19}};                     /* ragged / force_g == 32 */
static const Edge kOvl[] = {{256, 64, 4}, {1024, 64, 16}};
static const Edge kRagLocal[] = {{64, 16, 4}, {80, 16, 5}, {96, 16, 6}, {112, 16, 7}, {160, 16, 10}, {208, 16, 13}, {256, 16, 16}, {304, 16, 19},
                                 {320, 32, 10}, {384, 32, 12}, {416, 32, 13}, {512, 32, 16}, {608, 32, 19}};
static const Edge kRagGlobalFit[] = {{40, 8, 5}, {48, 8, 6}, {56, 8, 7}, {64, 8, 8}, {80, 8, 10}, {104, 8, 13}, {128, 8, 16}, {152, 8, 19},
                                     {160, 16, 10}, {208, 16, 13}, {256, 16, 16}, {304, 16, 19},
                                     {320, 32, 10}, {384, 32, 12}, {416, 32, 13}, {512, 32, 16}, {608, 32, 19}};
static const Edge kLaneWords[] = {{64, 1, 2}, {96, 1, 3}, {128, 1, 4}, {160, 1, 5}, {256, 1, 8}, {512, 1, 16}, {1024, 1, 32}};
static const Edge kGroupWords[] = {{1024, 32, 1}, {2048, 32, 2}, {4096, 32, 4}, {8192, 32, 8}, {16384, 32, 16}, {32768, 32, 32}};

static void check_tables()
{
	for (int l1 = 0; l1 <= 1100; ++l1) {
		CHECK(at::class_rows(at::kClass4, l1) == expect(kU4, l1).k, "4-lane groups, l1 = %d", l1);
		CHECK(at::class_rows(at::kClass8, l1) == expect(kG8, l1).k, "8-lane groups, l1 = %d", l1);
		CHECK(at::class_rows(at::kClass16, l1) == expect(kG16, l1).k, "16-lane groups, l1 = %d", l1);
		CHECK(at::class_rows(at::kClass32, l1) == expect(kG32, l1).k, "32-lane groups, l1 = %d", l1);
		CHECK(at::class_rows(at::kClass32, l1, 0, at::kClass32SkipUnderGroup32) == expect(kG32Group32, l1).k, "32-lane groups under AT_GROUP=32, l1 = %d", l1);
		CHECK(at::class_rows(at::kClass32, l1, at::kClass32RagFirst) == expect(kG32Rag, l1).k, "32-lane groups, ragged, l1 = %d", l1);
		CHECK(at::class_rows(at::kClassOvl, l1) == expect(kOvl, l1).k, "ragged overlap, l1 = %d", l1);
		CHECK(at::class_rows(at::kMyersLaneWords, l1) == expect(kLaneWords, l1).k, "bit-parallel words per lane, l1 = %d", l1);
		/* one strip: g * k rows hold the read */
		if (l1 <= 76) CHECK(4 * at::class_rows(at::kClass4, l1) >= l1, "l1 = %d", l1);
		if (l1 <= 152) CHECK(8 * at::class_rows(at::kClass8, l1) >= l1, "l1 = %d", l1);
		if (l1 <= 304) CHECK(16 * at::class_rows(at::kClass16, l1) >= l1, "l1 = %d", l1);
		if (l1 <= 608) {
			CHECK(32 * at::class_rows(at::kClass32, l1) >= l1, "l1 = %d", l1);
			CHECK(32 * at::class_rows(at::kClass32, l1, 0, at::kClass32SkipUnderGroup32) >= l1, "l1 = %d", l1);
			CHECK(32 * at::class_rows(at::kClass32, l1, at::kClass32RagFirst) >= l1, "l1 = %d", l1);
		}
		if (l1 <= 1024) CHECK(64 * at::class_rows(at::kClassOvl, l1) >= l1, "l1 = %d", l1);
		/* the five ragged modes: local, global, fit, overlap with tracebacks (the 64-lane group) and without (never in frames: the
		 * global / fit ladder, as before) */
		struct { int mode; bool ovl_tb; Edge e; } rag[5] = {
			{AT_MODE_LOCAL, false, expect(kRagLocal, l1)}, {AT_MODE_GLOBAL, false, expect(kRagGlobalFit, l1)}, {AT_MODE_FIT, false, expect(kRagGlobalFit, l1)},
			{AT_MODE_OVERLAP, true, expect(kOvl, l1)}, {AT_MODE_OVERLAP, false, expect(kRagGlobalFit, l1)}};
		for (const auto &r : rag) {
			const at::GroupRows c = at::rag_class(r.mode, r.ovl_tb, l1);
			CHECK(c.g == r.e.g && c.k == r.e.k, "rag_class(%d, %d, %d) = {%d, %d}, expected {%d, %d}", r.mode, (int)r.ovl_tb, l1, c.g, c.k, r.e.g, r.e.k);
			if (l1 <= at::one_strip_top(r.mode) && (r.mode != AT_MODE_OVERLAP || r.ovl_tb)) CHECK(c.g * c.k >= l1, "rag_class(%d, %d, %d)", r.mode, (int)r.ovl_tb, l1);
		}
	}
	for (int l1 = 0; l1 <= 40000; l1 += l1 < 1100 ? 1 : 97)
		CHECK(at::class_rows(at::kMyersGroupWords, l1) == expect(kGroupWords, l1).k, "bit-parallel words per lane of a 32-lane group, l1 = %d", l1);
	for (const Edge &e : kGroupWords) CHECK(at::class_rows(at::kMyersGroupWords, e.max_l1) == e.k && at::class_rows(at::kMyersGroupWords, e.max_l1 + 1) == expect(kGroupWords, e.max_l1 + 1).k, "edge %d", e.max_l1);
	CHECK(at::one_strip_top(AT_MODE_LOCAL) == 608 && at::one_strip_top(AT_MODE_GLOBAL) == 512 && at::one_strip_top(AT_MODE_FIT) == 416 &&
	      at::one_strip_top(AT_MODE_OVERLAP) == 1024, "one-strip tops");
	CHECK(at::kTopLocal == 608 && at::kTopGlobal == 512 && at::kTopFit == 416 && at::kTopOverlap == 1024, "one-strip tops");
	CHECK(at::rag_group_top(8) == 152 && at::rag_group_top(16) == 304 && at::rag_group_top(32) == 608 && at::rag_group_top(64) == 1024, "ragged tops");
	CHECK(sizeof at::kRagGroups / sizeof at::kRagGroups[0] == 4 && at::kRagGroups[0] == 8 && at::kRagGroups[1] == 16 && at::kRagGroups[2] == 32 &&
	      at::kRagGroups[3] == 64, "ragged group widths");
	/* s2 windows: 16 bases per word, two words of slack, odd stride */
	CHECK(at::myers_window_bytes(2, 0) == 24, "%zu", at::myers_window_bytes(2, 0));
	CHECK(at::myers_window_bytes(64, 150) == 3328, "%zu", at::myers_window_bytes(64, 150));
	CHECK(at::myers_window_bytes(64, 3792) == 61184 && at::myers_window_bytes(64, 3793) == 61696, "the 60 KB edge");
	CHECK(at::myers_window_bytes(8, 1000) == 8 * 65 * 4, "%zu", at::myers_window_bytes(8, 1000));
}

/* ---- seeded length sets (shared by the planner checks) ---- */
struct Rng {
	uint64_t s;
	explicit Rng(uint64_t seed) : s(seed * 0x9E3779B97F4A7C15ull + 0x1234567ull) {}
	uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
	int range(int lo, int hi) { return lo + (int)(next() % (uint32_t)(hi - lo + 1)); }   /* lo .. hi inclusive */
	template <size_t N> int pick(const int (&a)[N]) { return a[next() % N]; }
};

/* the read lengths of test_ragged_local_batches_in_frames, test_ragged_global_and_fit_batches_in_frames and
 * test_ragged_long_reads_in_32_lane_frames (tests/test_gpu_parity.py): both sides of every class edge */
static const int kLocalLens[] = {1, 2, 15, 16, 17, 40, 41, 48, 49, 56, 57, 63, 64, 65, 80, 81, 96, 104, 105, 112, 113, 128, 129, 150, 152, 160, 161, 207, 208,
                                 209, 250, 256, 257, 300, 304};
static const int kGlobalLens[] = {1, 2, 39, 40, 41, 48, 49, 56, 57, 64, 65, 80, 81, 104, 105, 128, 129, 150, 151, 152, 153, 160, 161, 200, 208, 209, 250, 256, 257, 300, 304};
static const int kLongLens[] = {150, 300, 304, 305, 306, 319, 320, 321, 383, 384, 385, 415, 416, 417, 500, 511, 512, 513, 600, 607, 608};

struct Case {
	const char *name;
	int mode;
	bool ovl_tb, frames;
	int64_t min_bucket;
	std::vector<int32_t> l1, l2;
};

static Case local_edges(const char *name, int n, int maxl, int64_t min_bucket, uint64_t seed)
{
	Case c{name, AT_MODE_LOCAL, false, true, min_bucket, {}, {}};
	Rng r(seed);
	for (int k = 0; k < n; ++k) {
		const int l1 = k % 3 == 0 ? r.pick(kLocalLens) : r.range(1, k % 2 ? 304 : 208);
		c.l1.push_back(std::min(l1, maxl));
		c.l2.push_back(r.range(1, 260));
	}
	return c;
}

static Case global_edges(const char *name, int mode, int n, uint64_t seed)
{
	static const int extra[] = {0, 5, 60, 300};
	Case c{name, mode, false, true, 16384, {}, {}};
	Rng r(seed);
	for (int k = 0; k < n; ++k) {
		const int l1 = k % 4 ? r.pick(kGlobalLens) : r.range(1, 304);
		c.l1.push_back(l1);
		c.l2.push_back(r.range(std::max(l1, 2), std::max(l1, 2) + r.pick(extra)));
	}
	return c;
}

static Case long_edges(const char *name, int mode, int n, int top, int64_t min_bucket, uint64_t seed)
{
	Case c{name, mode, false, true, min_bucket, {}, {}};
	Rng r(seed);
	for (int k = 0; k < n; ++k) {
		int l1;
		do l1 = k % 3 ? r.pick(kLongLens) : r.range(250, top); while (l1 > top);
		c.l1.push_back(l1);
		c.l2.push_back(mode == AT_MODE_FIT ? r.range(l1, l1 + 90) : r.range(std::max(1, l1 - 120), l1 + 120));
	}
	return c;
}

static Case uniform_random(const char *name, int mode, bool ovl_tb, bool frames, int n, int top1, int top2, int64_t min_bucket, uint64_t seed)
{
	Case c{name, mode, ovl_tb, frames, min_bucket, {}, {}};
	Rng r(seed);
	for (int k = 0; k < n; ++k) {
		const int l1 = r.range(1, top1);
		c.l1.push_back(l1);
		c.l2.push_back(mode == AT_MODE_FIT ? r.range(l1, l1 + top2) : r.range(1, top2));
	}
	return c;
}

/* the first eight are the ones whose plans are pinned by hash */
static std::vector<Case> all_cases()
{
	std::vector<Case> v;
	v.push_back(local_edges("local edges, 3000 pairs, min_bucket 16384", 3000, 304, 16384, 91));
	v.push_back(local_edges("local edges, 3000 pairs, min_bucket 1", 3000, 304, 1, 92));
	v.push_back(global_edges("global edges, 1400 pairs", AT_MODE_GLOBAL, 1400, 4471));
	v.push_back(global_edges("fit edges, 1400 pairs", AT_MODE_FIT, 1400, 4472));
	v.push_back(long_edges("local long edges, 260 pairs, min_bucket 64", AT_MODE_LOCAL, 260, 608, 64, 6085));
	v.push_back(long_edges("global long edges, 260 pairs", AT_MODE_GLOBAL, 260, 512, 16384, 6086));
	v.push_back(uniform_random("overlap with tracebacks, 500 pairs", AT_MODE_OVERLAP, true, true, 500, 1024, 1100, 16384, 9264));
	v.push_back(uniform_random("no frames, 5000 pairs", AT_MODE_GLOBAL, false, false, 5000, 2000, 2000, 16384, 77));
	/* invariants only */
	v.push_back(local_edges("local edges capped at 208", 3000, 208, 16384, 93));
	v.push_back(local_edges("local edges capped at 152, min_bucket 1", 3000, 152, 1, 94));
	v.push_back(long_edges("fit long edges, 260 pairs", AT_MODE_FIT, 260, 416, 16384, 6083));
	v.push_back(long_edges("local long edges, min_bucket 1", AT_MODE_LOCAL, 120, 608, 1, 6087));
	v.push_back(uniform_random("local, 5000 pairs, min_bucket 1", AT_MODE_LOCAL, false, true, 5000, 608, 700, 1, 5));
	v.push_back(uniform_random("local, 5000 pairs, min_bucket 16384", AT_MODE_LOCAL, false, true, 5000, 608, 700, 16384, 6));
	v.push_back(uniform_random("global, 5000 pairs", AT_MODE_GLOBAL, false, true, 5000, 512, 600, 16384, 7));
	v.push_back(uniform_random("fit, 64 pairs", AT_MODE_FIT, false, true, 64, 416, 200, 16384, 8));
	v.push_back(uniform_random("local, 64 pairs", AT_MODE_LOCAL, false, true, 64, 304, 300, 16384, 9));
	v.push_back(uniform_random("overlap with tracebacks, 64 pairs", AT_MODE_OVERLAP, true, true, 64, 1024, 1024, 16384, 10));
	{   /* one l1 occurs once: its work item is all padding but one entry */
		Case c = uniform_random("global, one l1 occurs once", AT_MODE_GLOBAL, false, true, 200, 1, 300, 16384, 11);
		for (auto &x : c.l1) x = 100;
		c.l1[57] = 37; c.l1[0] = 305; c.l1[199] = 153;
		v.push_back(c);
	}
	for (int mode : {AT_MODE_LOCAL, AT_MODE_GLOBAL, AT_MODE_FIT}) {   /* every l1 equal */
		Case c = uniform_random("all l1 equal", mode, false, true, 333, 1, 240, 1, 12 + mode);
		for (size_t k = 0; k < c.l1.size(); ++k) { c.l1[k] = 150; c.l2[k] += 150; }
		v.push_back(c);
	}
	v.push_back(uniform_random("no frames, local, 64 pairs", AT_MODE_LOCAL, false, false, 64, 900, 50, 16384, 13));
	return v;
}

static uint64_t fnv1a(uint64_t h, int64_t v, int bytes)
{
	for (int b = 0; b < bytes; ++b) { h ^= (uint64_t)(v >> (8 * b)) & 0xff; h *= 0x100000001b3ull; }
	return h;
}

/* ---- 2. the planner's invariants ---- */
static void check_plan(const Case &cs, const at::RagPlan &p)
{
	const int64_t n = (int64_t)cs.l1.size();
	const std::vector<int> &order = p.order;
	auto real = [&](size_t q) { return order[q] < 0 ? ~order[q] : order[q]; };
	auto cls = [&](int x) { return at::rag_class(cs.mode, cs.ovl_tb, cs.l1[(size_t)x]); };
	/* stripped of padding, a permutation of 0 .. n - 1; a padding entry repeats the last real entry before it */
	std::vector<int> seen((size_t)n, 0);
	size_t nreal = 0;
	for (size_t q = 0; q < order.size(); ++q) {
		if (order[q] >= 0) {
			CHECK(order[q] < n, "%s: order[%zu] = %d", cs.name, q, order[q]);
			if (order[q] < n) ++seen[(size_t)order[q]];
			++nreal;
		} else {
			size_t r = q;
			while (r > 0 && order[r] < 0) --r;
			CHECK(order[r] >= 0 && ~order[q] == order[r], "%s: padding entry %zu does not repeat the last real entry of its run", cs.name, q);
		}
	}
	CHECK(nreal == (size_t)n, "%s: %zu real entries for %lld pairs", cs.name, nreal, (long long)n);
	for (int64_t k = 0; k < n; ++k) CHECK(seen[(size_t)k] == 1, "%s: pair %lld appears %d times", cs.name, (long long)k, seen[(size_t)k]);
	if (!cs.frames) {
		CHECK(p.launches.empty() && order.size() == (size_t)n, "%s: launches without frames", cs.name);
		for (size_t q = 1; q < order.size(); ++q) {
			const int64_t a = (int64_t)cs.l1[(size_t)order[q - 1]] * cs.l2[(size_t)order[q - 1]], b = (int64_t)cs.l1[(size_t)order[q]] * cs.l2[(size_t)order[q]];
			CHECK(a > b || (a == b && order[q - 1] < order[q]), "%s: entry %zu out of order", cs.name, q);
		}
		return;
	}
	const bool local = cs.mode == AT_MODE_LOCAL;
	if (local) CHECK(order.size() == (size_t)n, "%s: local orders carry no padding", cs.name);
	/* the launches tile the order; every entry has its launch's class; f1 / f2 are the maxima */
	int64_t at = 0;
	for (size_t b = 0; b < p.launches.size(); ++b) {
		const at::RagLaunch &L = p.launches[b];
		CHECK(L.b0 == at && L.b1 > L.b0 && L.b1 <= (int64_t)order.size(), "%s: launch %zu is [%lld, %lld), expected to start at %lld", cs.name, b,
		      (long long)L.b0, (long long)L.b1, (long long)at);
		if (L.b0 != at || L.b1 <= L.b0 || L.b1 > (int64_t)order.size()) return;
		at = L.b1;
		const at::GroupRows c = cls(real((size_t)L.b0));
		int f1 = 0, f2 = 0;
		for (int64_t q = L.b0; q < L.b1; ++q) {
			const int x = real((size_t)q);
			CHECK(cls(x) == c && L.g == c.g, "%s: launch %zu entry %lld is of another class", cs.name, b, (long long)q);
			f1 = std::max(f1, cs.l1[(size_t)x]); f2 = std::max(f2, cs.l2[(size_t)x]);
		}
		CHECK(L.f1 == f1 && L.f2 == f2, "%s: launch %zu frame %dx%d, maxima %dx%d", cs.name, b, L.f1, L.f2, f1, f2);
		if (local) {
			/* (class descending, l2 descending, index) inside a launch */
			for (int64_t q = L.b0 + 1; q < L.b1; ++q) {
				const int x = order[(size_t)q - 1], y = order[(size_t)q];
				CHECK(cs.l2[(size_t)x] > cs.l2[(size_t)y] || (cs.l2[(size_t)x] == cs.l2[(size_t)y] && x < y), "%s: launch %zu entry %lld out of order", cs.name, b, (long long)q);
			}
			/* a bucket ends at a class change, or after min_bucket pairs once l2 is more than 20 % below the bucket's first */
			if (L.b1 < (int64_t)order.size()) {
				const int y = order[(size_t)L.b1];
				const bool class_change = cls(y) != c;
				const bool narrow = L.b1 - L.b0 >= cs.min_bucket && (int64_t)cs.l2[(size_t)y] * 5 < (int64_t)cs.l2[(size_t)order[(size_t)L.b0]] * 4;
				CHECK(class_change || narrow, "%s: launch %zu cut without a reason", cs.name, b);
				if (class_change) {
					const at::GroupRows d = cls(y);
					CHECK(d.g < c.g || (d.g == c.g && d.k < c.k), "%s: launch %zu: classes not in descending order", cs.name, b);
				}
			}
			/* ... and no sooner: no entry inside the bucket met the 20 % rule */
			for (int64_t q = L.b0 + cs.min_bucket; q < L.b1; ++q)
				CHECK((int64_t)cs.l2[(size_t)order[(size_t)q]] * 5 >= (int64_t)cs.l2[(size_t)order[(size_t)L.b0]] * 4, "%s: launch %zu runs past its cut", cs.name, b);
		} else {
			/* every aligned group of 2 * 64 / g entries has one l1; (l1 descending, l2 descending, index) over the real entries */
			const int64_t per = 2 * (64 / L.g);
			CHECK((L.b1 - L.b0) % per == 0, "%s: launch %zu is not whole work items", cs.name, b);   /* (items count from the launch's first entry) */
			for (int64_t q = L.b0; q < L.b1; ++q)
				CHECK(cs.l1[(size_t)real((size_t)q)] == cs.l1[(size_t)real((size_t)(q - (q - L.b0) % per))], "%s: work item at %lld mixes read lengths", cs.name, (long long)q);
			if (L.b1 < (int64_t)order.size()) CHECK(cls(real((size_t)L.b1)) != c, "%s: launch %zu cut inside a class", cs.name, b);
		}
	}
	CHECK(at == (int64_t)order.size(), "%s: launches end at %lld of %zu", cs.name, (long long)at, order.size());
	if (!local) {
		int prev = -1;
		for (size_t q = 0; q < order.size(); ++q) {
			if (order[q] < 0) continue;
			if (prev >= 0) {
				const int a1 = cs.l1[(size_t)prev], b1 = cs.l1[(size_t)order[q]], a2 = cs.l2[(size_t)prev], b2 = cs.l2[(size_t)order[q]];
				CHECK(a1 > b1 || (a1 == b1 && (a2 > b2 || (a2 == b2 && prev < order[q]))), "%s: entry %zu out of order", cs.name, q);
			}
			prev = order[q];
		}
		/* no more padding than one work item less one entry per distinct read length */
		std::vector<int> distinct((size_t)1101, 0);
		for (int v : cs.l1) distinct[(size_t)std::min(v, 1100)] = 1;
		size_t nd = 0;
		for (int v : distinct) nd += (size_t)v;
		CHECK(order.size() - (size_t)n <= nd * 15, "%s: %zu padding entries for %zu read lengths", cs.name, order.size() - (size_t)n, nd);
	}
}

/* ---- 3. the plans of the first eight cases, as the planning code inside align_host made them before the planner existed ---- */
static const uint64_t kPinned[8] = {
	0xc87319fa463a2587ull,   /* local edges, 3000 pairs, min_bucket 16384: 3000 entries, 8 launches */
	0x33bed92bf2bc9edaull,   /* local edges, 3000 pairs, min_bucket 1: 3000 entries, 136 launches */
	0x2e3d69e9778342f4ull,   /* global edges, 1400 pairs: 3528 entries, 12 launches */
	0xedcf7987f278e737ull,   /* fit edges, 1400 pairs: 3392 entries, 12 launches */
	0xe3362561ac81fabcull,   /* local long edges, 260 pairs, min_bucket 64: 260 entries, 8 launches */
	0x9bb1419c63a32558ull,   /* global long edges, 260 pairs: 532 entries, 7 launches */
	0x8db0ab4dafdea162ull,   /* overlap with tracebacks, 500 pairs: 822 entries, 2 launches */
	0x568dad0f17add281ull,   /* no frames, 5000 pairs: 5000 entries, 0 launches */
};

int main()
{
	check_tables();
	const std::vector<Case> cases = all_cases();
	for (size_t c = 0; c < cases.size(); ++c) {
		const Case &cs = cases[c];
		int max1 = 0, max2 = 0;
		for (size_t k = 0; k < cs.l1.size(); ++k) { max1 = std::max(max1, cs.l1[k]); max2 = std::max(max2, cs.l2[k]); }
		const at::RagPlan p = at::rag_plan(cs.mode, cs.ovl_tb, cs.l1.data(), cs.l2.data(), (int64_t)cs.l1.size(), max1, max2, cs.min_bucket, cs.frames);
		check_plan(cs, p);
		if (c < 8) {
			uint64_t h = 0xcbf29ce484222325ull;
			for (int x : p.order) h = fnv1a(h, x, 4);
			for (const at::RagLaunch &L : p.launches) { h = fnv1a(h, L.b0, 8); h = fnv1a(h, L.b1, 8); h = fnv1a(h, L.g, 4); h = fnv1a(h, L.f1, 4); h = fnv1a(h, L.f2, 4); }
			CHECK(h == kPinned[c], "%s: plan hash 0x%016llx, pinned 0x%016llx", cs.name, (unsigned long long)h, (unsigned long long)kPinned[c]);
		}
	}
	if (g_failures) { printf("ragplan_check: %d failures\n", g_failures); return 1; }
	printf("ragplan_check: ok (%zu plans)\n", cases.size());
	return 0;
}
