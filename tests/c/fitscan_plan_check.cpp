/*
 * fitscan_plan_check.cpp -- the fit scan's planner (csrc/at_fitscan_plan.h) without a GPU.  Built by `make asan` with
 * AddressSanitizer and UBSan and run by tests/test_fitscan_plan_check.py.  Over seeded (l1, l2, cutoff, tile_cols, scoring):
 *   1. the width is the caller's or the default; the overlap is the first multiple of 16 that holds l1 + g(l1, c) + 1, with
 *      c = max(cutoff, min(m, u) l1 + o + e), and does not shrink when the cutoff falls; the tiles are ceil(l2 / T), none for l2 < l1;
 *   2. every end column 0 .. l2 - 1 is owned by exactly one tile, and that tile -- or tile 0 for a tile that is not swept -- sweeps
 *      it as a column that is not its last; every sweep starts on a packed word; every swept tile has at least l1 and at least 2
 *      columns; the tiles 0 .. nfull - 1 have exactly T + ov columns, the others end in column l2 and have fewer;
 *   3. a hit's window: ws on a packed word, ws <= j* < we <= l2, we - ws >= l1, ws at or in front of
 *      j* - l1 - g(l1, score) - ceil(|o| / |e|) - 1 and less than 16 further;
 *   4. tile counts at l2 in {l1, l1 + 1, T, T + 1, 64 T, 64 T + 1, INT32_MAX}; the top and the bottom of the key's score field, its
 *      order (score, then M before L, then the column); the refusals.
 * Exit status 0 and "fitscan_plan_check: ok" when everything holds; every failure is printed.
 */
#include "../../aligntools/c_amd/csrc/at_fitscan_plan.h"

#include <climits>
#include <cstdio>
#include <initializer_list>

static int g_failures = 0;
#define CHECK(cond, ...)                                                        \
	do {                                                                        \
		if (!(cond)) {                                                          \
			if (++g_failures <= 40) { printf("FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
		}                                                                       \
	} while (0)

static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd()
{
	g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17;
	return g_state;
}
static int64_t between(int64_t lo, int64_t hi) { return lo + (int64_t)(rnd() % (uint64_t)(hi - lo + 1)); }

struct Sc { int m, u, o, e; };

static int64_t gap_of(int64_t l, int64_t s, Sc sc)
{
	const int64_t mx = sc.m > sc.u ? sc.m : sc.u, pen = -sc.o < -sc.e ? -sc.o : -sc.e;
	return mx * l - s > 0 ? (mx * l - s) / pen : 0;
}

static void check_one(int32_t l1, int32_t l2, int use_cutoff, int32_t cutoff, int32_t tile_cols, Sc s, bool walk_tiles)
{
	at::FitScanPlan p;
	const int rc = at::fitscan_plan(l1, l2, use_cutoff, cutoff, tile_cols, s.m, s.u, s.o, s.e, &p);
	CHECK(rc == AT_OK, "l1=%d l2=%d tile_cols=%d rc=%d", l1, l2, tile_cols, rc);
	if (rc != AT_OK) return;
	const int64_t lb = (int64_t)(s.m < s.u ? s.m : s.u) * l1 + s.o + s.e, c = use_cutoff && cutoff > lb ? cutoff : lb;
	const int64_t g = gap_of(l1, c, s);
	CHECK(at::fitscan_floor(l1, s.m, s.u, s.o, s.e) == lb && at::fitscan_bound(l1, use_cutoff, cutoff, s.m, s.u, s.o, s.e) == c, "lb=%lld c=%lld", (long long)lb, (long long)c);
	CHECK(p.tile == (tile_cols ? tile_cols : at::kFitScanDefaultTile) && p.tile % 16 == 0 && p.tile > 0, "tile=%d", p.tile);
	CHECK(p.overlap % 16 == 0 && p.overlap >= l1 + g + 1 && p.overlap < l1 + g + 1 + 16, "l1=%d g=%lld overlap=%d", l1, (long long)g, p.overlap);
	CHECK(p.ntiles == (l2 < l1 ? 0 : ((int64_t)l2 + p.tile - 1) / p.tile), "l1=%d l2=%d tile=%d tiles=%lld", l1, l2, p.tile, (long long)p.ntiles);
	CHECK(p.nfull >= 0 && p.nfull <= p.ntiles && (p.ntiles - p.nfull <= 1 || l2 < p.tile + p.overlap), "nfull=%lld of %lld", (long long)p.nfull, (long long)p.ntiles);
	/* monotone in the cutoff: a smaller bound never needs fewer columns */
	if (use_cutoff) {
		at::FitScanPlan q;
		CHECK(at::fitscan_plan(l1, l2, 1, cutoff - (int32_t)between(1, 50), tile_cols, s.m, s.u, s.o, s.e, &q) == AT_OK && q.overlap >= p.overlap, "overlap not monotone");
		CHECK(at::fitscan_plan(l1, l2, 0, 0, tile_cols, s.m, s.u, s.o, s.e, &q) == AT_OK && q.overlap >= p.overlap, "overlap without a cutoff is smaller");
	}
	if (walk_tiles && p.ntiles > 0) {
		const int64_t d = at::fitscan_dropped(l1, l2, p.tile, p.overlap);
		CHECK(d >= 0 && d <= p.ntiles - 1 && d == (p.overlap / p.tile < p.ntiles - 1 ? p.overlap / p.tile : p.ntiles - 1), "dropped=%lld of %lld", (long long)d, (long long)p.ntiles);
		int64_t at_col = 0;
		const int64_t e0 = at::fitscan_tile_end(0, p.tile, p.overlap, l2);
		for (int64_t n = 0; n < p.ntiles; ++n) {
			const int64_t s0 = at::fitscan_tile_start(n, p.tile, p.overlap), e = at::fitscan_tile_end(n, p.tile, p.overlap, l2);
			const int64_t lo = at::fitscan_own_lo(n, p.tile), hi = at::fitscan_own_hi(n, p.tile, l2);
			CHECK(lo == at_col && hi > lo, "tile %lld owns [%lld, %lld), expected from %lld", (long long)n, (long long)lo, (long long)hi, (long long)at_col);
			at_col = hi;
			if (n >= 1 && n <= d) {
				/* not swept: tile 0's end scan (the columns 0 .. e0 - 1) has its end columns */
				CHECK(s0 == 0 && e == e0 && hi <= e0, "dropped tile %lld: [%lld, %lld) against tile 0's (0, %lld]", (long long)n, (long long)lo, (long long)hi, (long long)e0);
				continue;
			}
			CHECK(s0 % 16 == 0 && s0 >= 0 && s0 == (lo - p.overlap > 0 ? lo - p.overlap : 0), "tile %lld sweeps from %lld", (long long)n, (long long)s0);
			/* the end scan of the pair (s0, e] covers the end columns s0 .. e - 1: the own range lies in it */
			CHECK(s0 <= lo && hi - 1 <= e - 1 && e <= l2 && e - s0 <= (int64_t)p.tile + p.overlap, "tile %lld sweeps (%lld, %lld], owns up to %lld", (long long)n, (long long)s0, (long long)e, (long long)hi);
			CHECK(e - s0 >= l1 && (e - s0 >= 2 || l2 < 2), "tile %lld has %lld columns for %d rows", (long long)n, (long long)(e - s0), l1);
			if (n < p.nfull) CHECK(e - s0 == (int64_t)p.tile + p.overlap, "full tile %lld has %lld columns", (long long)n, (long long)(e - s0));
			else CHECK(e == l2 && e - s0 < (int64_t)p.tile + p.overlap, "short tile %lld has %lld columns up to %lld", (long long)n, (long long)(e - s0), (long long)e);
			/* a path that scores >= c and ends in an own column starts behind s0, or the tile starts with the target */
			CHECK(s0 == 0 || lo - s0 >= l1 + g + 1, "tile %lld: %lld columns in front of its own range", (long long)n, (long long)(lo - s0));
		}
		CHECK(at_col == l2, "covered %lld of %d", (long long)at_col, l2);
		const int64_t ns = at::fitscan_swept(l1, l2, p.tile, p.overlap), nfs = at::fitscan_swept_full(l1, l2, p.tile, p.overlap);
		CHECK(ns == p.ntiles - d && nfs >= 0 && nfs <= ns, "swept=%lld full=%lld", (long long)ns, (long long)nfs);
		for (int64_t k = 0; k < ns; ++k) {
			const int64_t n = at::fitscan_swept_tile(k, d);
			CHECK(n < p.ntiles && (k == 0 ? n == 0 : n == k + d), "swept tile %lld is tile %lld", (long long)k, (long long)n);
			CHECK((n < p.nfull) == (k < nfs), "swept tile %lld (tile %lld): full=%d, among the first %lld", (long long)k, (long long)n, (int)(n < p.nfull), (long long)nfs);
		}
	}
	if (l2 < l1) {
		CHECK(at::fitscan_swept(l1, l2, p.tile, p.overlap) == 0 && at::fitscan_swept_full(l1, l2, p.tile, p.overlap) == 0 && p.nfull == 0, "a target shorter than the query has tiles");
		return;
	}
	const int64_t mx = s.m > s.u ? s.m : s.u;
	for (int q = 0; q < 4 && l2 > 1; ++q) {
		const int32_t score = (int32_t)between(lb - 40, mx * l1);
		const int64_t js = q == 0 ? l2 - 1 : between(1, l2 - 1);
		const int64_t ws = at::fitscan_window_start(js, l1, score, s.m, s.u, s.o, s.e), we = at::fitscan_window_end(js, ws, l1, l2);
		const int64_t want = js - l1 - gap_of(l1, score, s) - ((-s.o) + (-s.e) - 1) / (-s.e) - 1;
		CHECK(ws % 16 == 0 && ws >= 0 && ws <= js && js < we && we <= l2, "ws=%lld j*=%lld we=%lld l2=%d", (long long)ws, (long long)js, (long long)we, l2);
		CHECK(we - ws >= l1 && (we == js + 1 || we == ws + l1), "ws=%lld we=%lld l1=%d j*=%lld", (long long)ws, (long long)we, l1, (long long)js);
		CHECK(want <= 0 ? ws == 0 : (ws <= want && want - ws < 16), "ws=%lld want=%lld", (long long)ws, (long long)want);
	}
}

int main()
{
	const Sc scs[] = {{2, -2, -5, -2}, {1, -2, -5, -1}, {5, -4, -10, -1}, {3, -1, -1, -3}, {1, 3, -1, -1}, {2, -6, -2, -1}};
	const int32_t widths[] = {0, 16, 32, 48, 256, 1024, 4096};
	const int32_t cutoffs[] = {-3000, -40, 0, 3, 40, 300, 5000};
	/* tile counts at the edges */
	for (int32_t T : {16, 48, 256, 2048}) {
		for (int32_t l1 : {1, 20, 150, 1024}) {
			const int32_t l2s[] = {l1, l1 + 1, T, T + 1, 64 * T, 64 * T + 1};
			for (int x = 0; x < 6; ++x) {
				const int32_t l2 = l2s[x];
				at::FitScanPlan p;
				const int64_t want = l2 < l1 ? 0 : ((int64_t)l2 + T - 1) / T;
				CHECK(at::fitscan_plan(l1, l2, 0, 0, T, 2, -2, -5, -2, &p) == AT_OK && p.ntiles == want, "T=%d l1=%d l2=%d tiles=%lld", T, l1, l2, (long long)p.ntiles);
				for (int uc = 0; uc < 2; ++uc) check_one(l1, l2, uc, 12, T, scs[x % 6], true);
			}
		}
		at::FitScanPlan p;
		CHECK(at::fitscan_plan(150, T, 0, 0, T, 2, -2, -5, -2, &p) == AT_OK && p.ntiles == (T < 150 ? 0 : 1), "T=%d l2=T", T);
		CHECK(at::fitscan_plan(150, INT32_MAX, 0, 0, T, 2, -2, -5, -2, &p) == AT_OK && p.ntiles == ((int64_t)INT32_MAX + T - 1) / T, "T=%d l2=INT32_MAX", T);
		/* the last tiles of the longest target */
		for (int64_t n = p.ntiles - 3; n < p.ntiles; ++n) {
			const int64_t s0 = at::fitscan_tile_start(n, p.tile, p.overlap), e = at::fitscan_tile_end(n, p.tile, p.overlap, INT32_MAX);
			CHECK(s0 >= 0 && s0 % 16 == 0 && e - s0 >= 150 && e <= INT32_MAX && e >= at::fitscan_own_hi(n, p.tile, INT32_MAX), "tile %lld of INT32_MAX: (%lld, %lld]", (long long)n, (long long)s0, (long long)e);
		}
		CHECK(at::fitscan_tile_end(p.ntiles - 1, p.tile, p.overlap, INT32_MAX) == INT32_MAX, "the last tile ends in l2");
	}
	for (int n = 0; n < 4000; ++n) {
		const Sc s = scs[rnd() % 6];
		const int32_t l1 = (int32_t)between(1, 1024);
		const bool big = n % 50 == 0;
		const int32_t l2 = big ? (int32_t)between(2000000000, 2147483647) : n % 7 == 0 ? (int32_t)between(0, 2 * l1) : (int32_t)between(0, 100000);
		const int32_t T = big ? 4096 * 16 : widths[rnd() % 7];
		check_one(l1, l2, (int)(rnd() & 1), cutoffs[rnd() % 7], T, s, !big || n % 500 == 0);
	}
	/* hand-computed: 150 rows, 2/-2/-5/-2: lb = -300 - 7, g = floor((300 + 307) / 2) = 303, ov = round16up(454) = 464 */
	{
		at::FitScanPlan p;
		CHECK(at::fitscan_plan(150, 300000, 0, 0, 0, 2, -2, -5, -2, &p) == AT_OK && p.tile == 1024 && p.overlap == 464 && p.ntiles == 293 && p.nfull == 292, "150 x 300000: %d %d %lld %lld", p.tile, p.overlap, (long long)p.ntiles, (long long)p.nfull);
		CHECK(at::fitscan_plan(150, 300000, 1, 150, 0, 2, -2, -5, -2, &p) == AT_OK && p.overlap == 240, "cutoff 150: overlap=%d", p.overlap);
		CHECK(at::fitscan_plan(150, 300000, 1, -100000, 0, 2, -2, -5, -2, &p) == AT_OK && p.overlap == 464, "a cutoff under lb: overlap=%d", p.overlap);
	}
	/* the key: the whole int32 range but INT32_MIN; score first, then M before L, then the column; no result is the empty slot */
	{
		const unsigned long long top = at::fitscan_key(INT32_MAX, 0, 0), bot = at::fitscan_key(-INT32_MAX, 1, INT32_MAX);
		CHECK(top == 0 && bot == ~0ull - (1ull << 32) && bot < ~0ull, "top=%llx bottom=%llx", top, bot);
		CHECK(at::fitscan_key_score(top) == INT32_MAX && at::fitscan_key_low(top) == 0 && at::fitscan_key_end_j(top) == 0, "top parts");
		CHECK(at::fitscan_key_score(bot) == -INT32_MAX && at::fitscan_key_low(bot) == 1 && at::fitscan_key_end_j(bot) == INT32_MAX, "bottom parts");
		CHECK(at::fitscan_key_ok(INT32_MAX, 0) && at::fitscan_key_ok(-(int64_t)INT32_MAX, INT32_MAX) && !at::fitscan_key_ok(INT32_MIN, 0) &&
		      !at::fitscan_key_ok(0, -1) && !at::fitscan_key_ok(0, (int64_t)INT32_MAX + 1) && !at::fitscan_key_ok((int64_t)INT32_MAX + 1, 0), "key_ok");
		CHECK(at::fitscan_key(-5, 1, 9) < at::fitscan_key(-6, 0, 1) && at::fitscan_key(-5, 0, 9) < at::fitscan_key(-5, 1, 1) &&
		      at::fitscan_key(-5, 1, 9) < at::fitscan_key(-5, 1, 10) && at::fitscan_key(3, 0, 7) < at::fitscan_key(-3, 0, 7) && at::fitscan_key(0, 0, 5) < at::fitscan_key(-1, 0, 4), "key order");
		for (int n = 0; n < 2000; ++n) {
			const int32_t sc = (int32_t)between(-INT32_MAX, INT32_MAX), j = (int32_t)between(0, INT32_MAX);
			const int low = (int)(rnd() & 1);
			const unsigned long long k = at::fitscan_key(sc, low, j);
			CHECK(at::fitscan_key_score(k) == sc && at::fitscan_key_low(k) == low && at::fitscan_key_end_j(k) == j && k != ~0ull, "key parts of %d %d %d", sc, low, j);
		}
	}
	at::FitScanPlan p;
	for (int32_t bad : {24, 8, -16, 1000, 17}) CHECK(at::fitscan_plan(10, 100, 0, 0, bad, 2, -2, -5, -2, &p) == AT_ERR_ARG, "tile_cols=%d accepted", bad);
	CHECK(at::fitscan_plan(-1, 100, 0, 0, 16, 2, -2, -5, -2, &p) == AT_ERR_ARG && at::fitscan_plan(1, -100, 0, 0, 16, 2, -2, -5, -2, &p) == AT_ERR_ARG, "negative length accepted");
	CHECK(at::fitscan_plan(10, 100, 0, 0, 16, 0, -2, -5, -2, &p) == AT_ERR_DOMAIN, "m = 0 accepted");
	CHECK(at::fitscan_plan(10, 100, 0, 0, 16, 2, -2, 0, -2, &p) == AT_ERR_DOMAIN, "o = 0 accepted");
	CHECK(at::fitscan_plan(10, 100, 0, 0, 16, 2, -2, -5, 0, &p) == AT_ERR_DOMAIN, "e = 0 accepted");
	CHECK(at::fitscan_plan(10, 100, 0, 0, 16, 2, -2, -5, 1, &p) == AT_ERR_DOMAIN, "e = 1 accepted");
	CHECK(at::fitscan_plan(0, 100, 0, 0, 16, 2, -2, -5, -2, &p) == AT_ERR_DOMAIN, "an empty query accepted");
	CHECK(at::fitscan_plan(1025, 100, 0, 0, 16, 2, -2, -5, -2, &p) == AT_ERR_DOMAIN, "a 1 025-base query accepted");
	CHECK(at::fitscan_plan(1024, 100, 0, 0, 16, 2, 7, -5, -2, &p) == AT_OK, "u > m refused");
	/* |u| is anything: an overlap past int32 is refused, and nothing wraps on the way */
	CHECK(at::fitscan_plan(1024, 100, 0, 0, 16, 1, INT32_MIN + 1, -1, -1, &p) == AT_ERR_DOMAIN, "an overlap past 2^31 accepted");
	CHECK(at::fitscan_overlap(1024, 0, 0, 1, INT32_MIN + 1, -1, -1) > INT32_MAX, "the overlap is 64 bits wide");
	CHECK(at::fitscan_plan(1024, 100, 1, INT32_MAX, 16, 1, INT32_MIN + 1, -1, -1, &p) == AT_OK && p.overlap == 1040, "the cutoff bounds the overlap: %d", p.overlap);
	if (g_failures) { printf("fitscan_plan_check: %d failures\n", g_failures); return 1; }
	printf("fitscan_plan_check: ok\n");
	return 0;
}
