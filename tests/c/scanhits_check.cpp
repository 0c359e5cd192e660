/*
 * scanhits_check.cpp -- the selection rule of at_scan_hits (csrc/at_scanhits.h) without a GPU.  Built by `make asan` with
 * AddressSanitizer and UBSan and run by tests/test_scan_hits_check.py.  Over seeded pairs on ACGT / AC / A with planted, mutated copies:
 *   1. the last row of the infix table by the recurrence; the occurrences by the DEFINITION (first column of a run of equal values
 *      that is at or under c, below the run in front of it and the last run or below the run behind it);
 *   2. the descents S at or under c of several pairs as candidate records -- runs of descents in consecutive columns, cut at random as
 *      tile borders cut them, or every descent alone --, shuffled as the appends of a sweep land, sorted by key: scan_is_valley marks
 *      exactly the occurrences, never looking past its pair;
 *   3. scan_hit_kept against the separation's definition (no OTHER OCCURRENCE within sep columns with a smaller (v, a)), for
 *      sep = 0, small, the read's length (AT_SCAN_SEP_READ) and larger than the target;
 *   4. the candidates of the tiles of the planner (at_scanplan.h, cutoff c), each tile's own table, are S;
 *   5. scan_hits_order sorts by (query, distance, target, strand, column) and is a permutation.
 * Exit status 0 and "scanhits_check: ok" when everything holds; every failure is printed.
 */
#include "../../aligntools/c_amd/csrc/at_scanhits.h"
#include "../../aligntools/c_amd/csrc/at_scanplan.h"

#include <cstdio>
#include <string>
#include <utility>
#include <vector>

static int g_failures = 0;
#define CHECK(cond, ...)                                                        \
	do {                                                                        \
		if (!(cond)) {                                                          \
			if (++g_failures <= 40) { printf("FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
		}                                                                       \
	} while (0)

static uint64_t g_state = 0x2545f4914f6cdd1dull;
static uint64_t rnd()
{
	g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17;
	return g_state;
}
static int64_t between(int64_t lo, int64_t hi) { return lo + (int64_t)(rnd() % (uint64_t)(hi - lo + 1)); }

static std::string random_seq(int n, const char *alpha, int na)
{
	std::string s((size_t)n, 'A');
	for (char &c : s) c = alpha[rnd() % (uint64_t)na];
	return s;
}

/* D(l1, 0 .. l2) of q inside t */
static std::vector<int32_t> last_row(const std::string &q, const std::string &t)
{
	const size_t l1 = q.size(), l2 = t.size();
	std::vector<int32_t> prev(l2 + 1, 0), cur(l2 + 1, 0);
	for (size_t i = 1; i <= l1; ++i) {
		cur[0] = (int32_t)i;
		for (size_t j = 1; j <= l2; ++j) {
			const int32_t a = prev[j - 1] + (q[i - 1] != t[j - 1]), b = prev[j] + 1, c = cur[j - 1] + 1;
			cur[j] = std::min(a, std::min(b, c));
		}
		prev.swap(cur);
	}
	return prev;
}

typedef std::pair<int64_t, int32_t> Occ;   /* (column, value) */

static std::vector<Occ> occurrences(const std::vector<int32_t> &row, int32_t c)
{
	std::vector<Occ> out;
	const int64_t l2 = (int64_t)row.size() - 1;
	for (int64_t a = 1; a <= l2; ++a) {
		const int32_t v = row[(size_t)a];
		if (v > c || row[(size_t)a - 1] <= v) continue;
		int64_t b = a;
		while (b < l2 && row[(size_t)b + 1] == v) ++b;
		if (b == l2 || row[(size_t)b + 1] > v) out.push_back(Occ(a, v));
	}
	return out;
}

static std::vector<Occ> descents(const std::vector<int32_t> &row, int32_t c, int64_t first, int64_t base)
{
	std::vector<Occ> out;
	for (int64_t j = first; j < (int64_t)row.size(); ++j)
		if (row[(size_t)j] <= c && row[(size_t)j] < row[(size_t)j - 1]) out.push_back(Occ(base + j, row[(size_t)j]));
	return out;
}

static std::vector<Occ> separated(const std::vector<Occ> &occ, int64_t sep)
{
	std::vector<Occ> out;
	for (size_t i = 0; i < occ.size(); ++i) {
		bool beaten = false;
		for (size_t x = 0; x < occ.size() && sep > 0; ++x) {
			if (x == i) continue;
			const int64_t d = occ[x].first > occ[i].first ? occ[x].first - occ[i].first : occ[i].first - occ[x].first;
			if (d <= sep && (occ[x].second < occ[i].second || (occ[x].second == occ[i].second && occ[x].first < occ[i].first))) beaten = true;
		}
		if (!beaten) out.push_back(occ[i]);
	}
	return out;
}

struct Pair { std::string q, t; int32_t max_dist; std::vector<int32_t> row; };

static Pair make_pair(int n)
{
	static const char *alphas[4] = {"ACGT", "ACGT", "AC", "A"};
	static const int nas[4] = {4, 4, 2, 1};
	const char *alpha = alphas[n % 4];
	const int na = nas[n % 4];
	Pair p;
	const int l1 = n % 13 ? (int)between(1, 45) : (int)between(60, 90);
	const int l2 = n % 17 == 0 ? (int)between(0, 17) : (int)between(0, 400);
	p.q = random_seq(l1, alpha, na);
	p.t = random_seq(l2, alpha, na);
	for (int k = (int)between(0, 3); k > 0 && l2 > 0; --k) {
		std::string body = p.q;
		for (int e = (int)between(0, 4); e > 0; --e) body[(size_t)between(0, (int64_t)body.size() - 1)] = alpha[rnd() % (uint64_t)na];
		if (body.size() > 1 && rnd() % 5 < 2) body.erase((size_t)between(0, (int64_t)body.size() - 1), 1);
		const size_t at = (size_t)between(0, std::max<int64_t>(0, l2 - (int64_t)body.size()));
		for (size_t x = 0; x < body.size() && at + x < p.t.size(); ++x) p.t[at + x] = body[x];
	}
	p.max_dist = (int32_t)between(0, 45);
	p.row = last_row(p.q, p.t);
	return p;
}

int main()
{
	long long nocc = 0, nkept_less = 0, ntiles = 0, nruns_longer = 0;
	/* batches of pairs share one candidate list, as the pairs of a slice do */
	for (int batch = 0; batch < 80; ++batch) {
		const int np = (int)between(1, 7);
		std::vector<Pair> pairs;
		for (int x = 0; x < np; ++x) pairs.push_back(make_pair(batch * 7 + x));
		std::vector<std::pair<uint64_t, int32_t>> cand;
		for (int x = 0; x < np; ++x) {
			const Pair &p = pairs[(size_t)x];
			const int32_t l1 = (int32_t)p.q.size(), c = at::scan_hits_bound(l1, p.max_dist);
			CHECK(c == std::min(p.max_dist, l1 - 1) && c < l1, "c=%d", c);
			const std::vector<Occ> S = descents(p.row, c, 1, 0);
			/* runs of descents in consecutive columns, cut at random as tile borders cut them; every fourth batch leaves each descent alone */
			for (size_t k = 0; k < S.size();) {
				size_t e = k;
				while (e + 1 < S.size() && S[e + 1].first == S[e].first + 1 && batch % 4 != 0 && rnd() % 3 != 0) ++e;
				CHECK(S[e].second == S[k].second - (int32_t)(e - k), "a run of descents falls by one per column");
				cand.push_back(std::make_pair(at::scan_cand_key(x, S[e].first), at::scan_cand_val(S[e].second, S[k].second)));
				nruns_longer += e > k;
				k = e + 1;
			}
			/* 4. the tiles of the planner see exactly S */
			const int32_t T = 16 << (batch % 3);
			at::ScanPlan plan;
			CHECK(at::scan_plan(l1, (int32_t)p.t.size(), 1, c, T, &plan) == AT_OK && plan.overlap == ((l1 + c + 15) & ~15), "plan");
			std::vector<Occ> seen;
			for (int64_t n = 0; n < 64 * plan.ngroups; ++n) {
				const int64_t s0 = at::scan_tile_start(n, T, plan.overlap), e = at::scan_tile_end(n, T, (int32_t)p.t.size());
				if (e <= n * T) break;
				++ntiles;
				const std::vector<int32_t> tr = last_row(p.q, p.t.substr((size_t)s0, (size_t)(e - s0)));
				const std::vector<Occ> mine = descents(tr, c, n * T - s0 + 1, s0);
				seen.insert(seen.end(), mine.begin(), mine.end());
			}
			CHECK(seen == S, "batch %d pair %d: %zu candidates from the tiles, %zu in the row", batch, x, seen.size(), S.size());
		}
		/* the appends land in any order; the keys are unique */
		for (size_t i = cand.size(); i > 1; --i) std::swap(cand[i - 1], cand[(size_t)between(0, (int64_t)i - 1)]);
		std::sort(cand.begin(), cand.end());
		std::vector<uint64_t> key;
		std::vector<int32_t> val;
		for (const auto &k : cand) { key.push_back(k.first); val.push_back(k.second); }
		for (size_t i = 1; i < key.size(); ++i) CHECK(key[i - 1] < key[i], "keys not unique at %zu", i);
		const int64_t n = (int64_t)key.size();
		for (int x = 0; x < np; ++x) {
			const Pair &p = pairs[(size_t)x];
			const int32_t l1 = (int32_t)p.q.size(), c = at::scan_hits_bound(l1, p.max_dist);
			const std::vector<Occ> occ = occurrences(p.row, c);
			nocc += (long long)occ.size();
			/* 2. valleys */
			std::vector<Occ> got;
			for (int64_t i = 0; i < n; ++i)
				if (at::scan_cand_pair(key[(size_t)i]) == x && at::scan_is_valley(key.data(), val.data(), n, i))
					got.push_back(Occ(at::scan_cand_column(key[(size_t)i]), at::scan_cand_tail(val[(size_t)i])));
			CHECK(got == occ, "batch %d pair %d: %zu valleys, %zu occurrences", batch, x, got.size(), occ.size());
			/* 3. separation */
			const int32_t seps[5] = {0, 1, (int32_t)between(2, 12), AT_SCAN_SEP_READ, 100000};
			for (int32_t ms : seps) {
				const int64_t sep = at::scan_hits_sep(ms, l1);
				CHECK(sep == (ms == AT_SCAN_SEP_READ ? l1 : ms), "sep");
				const std::vector<Occ> want = separated(occ, sep);
				std::vector<Occ> kept;
				for (int64_t i = 0; i < n; ++i)
					if (at::scan_cand_pair(key[(size_t)i]) == x && at::scan_hit_kept(key.data(), val.data(), n, i, sep))
						kept.push_back(Occ(at::scan_cand_column(key[(size_t)i]), at::scan_cand_tail(val[(size_t)i])));
				CHECK(kept == want, "batch %d pair %d sep %lld: %zu kept, %zu by the definition", batch, x, (long long)sep, kept.size(), want.size());
				if (ms == 0) CHECK(kept == occ, "sep 0 keeps every occurrence");
				nkept_less += kept.size() < occ.size();
			}
		}
	}
	/* a single candidate */
	{
		const uint64_t k1[1] = {at::scan_cand_key(3, 9)};
		const int32_t v1[1] = {at::scan_cand_val(2, 5)};
		CHECK(at::scan_cand_tail(v1[0]) == 2 && at::scan_cand_head(v1[0]) == 5 && at::scan_cand_head(at::scan_cand_val(1023, 1024)) == 1024, "value fields");
		CHECK(at::scan_is_valley(k1, v1, 1, 0) && at::scan_hit_kept(k1, v1, 1, 0, 1000), "a single candidate is a kept occurrence");
		CHECK(at::scan_cand_pair(k1[0]) == 3 && at::scan_cand_column(k1[0]) == 9, "key fields");
		const uint64_t big = at::scan_cand_key((1LL << 28) - 1, 0x7fffffff);
		CHECK(at::scan_cand_pair(big) == (1LL << 28) - 1 && at::scan_cand_column(big) == 0x7fffffff, "key fields at their limits");
	}
	/* 5. the order */
	{
		std::vector<at::ScanHit> hits;
		for (int x = 0; x < 3000; ++x)
			hits.push_back({(int32_t)between(0, 5), (int32_t)between(0, 3), (int32_t)between(0, 1), (int32_t)between(0, 4), (int32_t)between(1, 50)});
		long long sum = 0, after = 0;
		for (const at::ScanHit &x : hits) sum += x.query * 1000003LL + x.target * 10007LL + x.strand * 101LL + x.score * 13LL + x.end_j;
		at::scan_hits_order(hits.data(), (int64_t)hits.size());
		for (const at::ScanHit &x : hits) after += x.query * 1000003LL + x.target * 10007LL + x.strand * 101LL + x.score * 13LL + x.end_j;
		CHECK(sum == after, "not a permutation");
		for (size_t i = 1; i < hits.size(); ++i) {
			const at::ScanHit &a = hits[i - 1], &b = hits[i];
			const long long ka[5] = {a.query, a.score, a.target, a.strand, a.end_j}, kb[5] = {b.query, b.score, b.target, b.strand, b.end_j};
			bool le = true;
			for (int f = 0; f < 5; ++f) { if (ka[f] != kb[f]) { le = ka[f] < kb[f]; break; } }
			CHECK(le, "order broken at %zu", i);
		}
		at::scan_hits_order(nullptr, 0);
	}
	CHECK(nocc > 1000 && nkept_less > 100 && ntiles > 2000 && nruns_longer > 500, "too little covered: %lld occurrences, %lld thinned lists, %lld tiles, %lld runs of several descents",
	      nocc, nkept_less, ntiles, nruns_longer);
	if (g_failures) { printf("scanhits_check: %d failures\n", g_failures); return 1; }
	printf("scanhits_check: ok (%lld occurrences, %lld tiles)\n", nocc, ntiles);
	return 0;
}
