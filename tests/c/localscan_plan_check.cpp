/*
 * localscan_plan_check.cpp -- the local scan's planner (csrc/at_localscan_plan.h) without a GPU.  Built by `make asan` with
 * AddressSanitizer and UBSan and run by tests/test_localscan_plan_check.py.  Over seeded (l1, l2, cutoff, tile_cols, scoring):
 *   1. the width is the caller's or the default; the overlap is the first multiple of 16 that holds l1 + g(l1, c) and does not
 *      shrink when the cutoff falls; the tiles are ceil(l2 / T);
 *   2. the own ranges of the tiles cover the columns 1 .. l2 exactly once and in order; every sweep starts on a packed word, at
 *      max(0, n T - ov), and reaches its own range's end; the tiles 0 .. nfull - 1 have exactly T + ov columns, the others end in
 *      column l2 and have fewer;
 *   3. a hit's window starts on a packed word, at or in front of j* - i* - g(i*, score) - ceil(|o| / |e|) - 1, less than 16 further;
 *   4. tile counts at l2 in {0, 1, T, T + 1, 64 T, 64 T + 1, INT32_MAX}; no overflow at l1 = 1 024 with m = 1 023; the key's parts
 *      come back; the domain refusals.
 * Exit status 0 and "localscan_plan_check: ok" when everything holds; every failure is printed.
 */
#include "../../aligntools/c_amd/csrc/at_localscan_plan.h"

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

static void check_one(int32_t l1, int32_t l2, int use_cutoff, int32_t cutoff, int32_t tile_cols, Sc s, bool walk_tiles)
{
	at::LocalScanPlan p;
	const int rc = at::localscan_plan(l1, l2, use_cutoff, cutoff, tile_cols, s.m, s.u, s.o, s.e, &p);
	CHECK(rc == AT_OK, "l1=%d l2=%d tile_cols=%d rc=%d", l1, l2, tile_cols, rc);
	if (rc != AT_OK) return;
	const int64_t mx = s.m > s.u ? s.m : s.u, pen = -s.o < -s.e ? -s.o : -s.e, c = use_cutoff && cutoff > 1 ? cutoff : 1;
	const int64_t g = mx * l1 - c > 0 ? (mx * l1 - c) / pen : 0;
	CHECK(p.tile == (tile_cols ? tile_cols : at::kLocalScanDefaultTile) && p.tile % 16 == 0 && p.tile > 0, "tile=%d", p.tile);
	CHECK(p.overlap % 16 == 0 && p.overlap >= l1 + g && p.overlap < l1 + g + 16, "l1=%d g=%lld overlap=%d", l1, (long long)g, p.overlap);
	CHECK(p.ntiles == ((int64_t)l2 + p.tile - 1) / p.tile, "l2=%d tile=%d tiles=%lld", l2, p.tile, (long long)p.ntiles);
	CHECK(p.nfull >= 0 && p.nfull <= p.ntiles && (p.ntiles - p.nfull <= 1 || l2 < p.tile + p.overlap), "nfull=%lld of %lld", (long long)p.nfull, (long long)p.ntiles);
	/* monotone in the cutoff: a smaller bound never needs fewer columns */
	if (use_cutoff) {
		at::LocalScanPlan q;
		CHECK(at::localscan_plan(l1, l2, 1, cutoff - (int32_t)between(1, 50), tile_cols, s.m, s.u, s.o, s.e, &q) == AT_OK && q.overlap >= p.overlap, "overlap not monotone");
		CHECK(at::localscan_plan(l1, l2, 0, 0, tile_cols, s.m, s.u, s.o, s.e, &q) == AT_OK && q.overlap >= p.overlap, "overlap without a cutoff is smaller");
	}
	if (walk_tiles) {
		int64_t at_col = 0;
		for (int64_t n = 0; n < p.ntiles; ++n) {
			const int64_t s0 = at::localscan_tile_start(n, p.tile, p.overlap), e = at::localscan_tile_end(n, p.tile, p.overlap, l2);
			const int64_t lo = at::localscan_own_lo(n, p.tile), hi = at::localscan_own_hi(n, p.tile, l2);
			CHECK(lo == at_col && hi > lo, "tile %lld owns (%lld, %lld], expected from %lld", (long long)n, (long long)lo, (long long)hi, (long long)at_col);
			CHECK(s0 % 16 == 0 && s0 >= 0 && s0 == (lo - p.overlap > 0 ? lo - p.overlap : 0), "tile %lld sweeps from %lld", (long long)n, (long long)s0);
			CHECK(e >= hi && e <= l2 && e - s0 <= (int64_t)p.tile + p.overlap, "tile %lld sweeps (%lld, %lld], owns up to %lld", (long long)n, (long long)s0, (long long)e, (long long)hi);
			if (n < p.nfull) CHECK(e - s0 == (int64_t)p.tile + p.overlap, "full tile %lld has %lld columns", (long long)n, (long long)(e - s0));
			else CHECK(e == l2 && e - s0 < (int64_t)p.tile + p.overlap, "short tile %lld has %lld columns up to %lld", (long long)n, (long long)(e - s0), (long long)e);
			at_col = hi;
		}
		CHECK(at_col == l2, "covered %lld of %d", (long long)at_col, l2);
		/* the tiles that are not swept repeat tile 0's columns exactly, every other tile differs from tile 0; the swept tiles in order */
		const int64_t d = at::localscan_dropped(l2, p.tile, p.overlap);
		CHECK(d >= 0 && (p.ntiles == 0 ? d == 0 : d <= p.ntiles - 1), "dropped=%lld of %lld", (long long)d, (long long)p.ntiles);
		for (int64_t n = 1; n < p.ntiles; ++n) {
			const bool same = at::localscan_tile_start(n, p.tile, p.overlap) == 0 &&
			                  at::localscan_tile_end(n, p.tile, p.overlap, l2) == at::localscan_tile_end(0, p.tile, p.overlap, l2);
			CHECK(same == (n <= d) || (same && n > d && at::localscan_tile_end(n, p.tile, p.overlap, l2) == l2), "tile %lld: repeat=%d, dropped=%lld", (long long)n, (int)same, (long long)d);
			if (n <= d) CHECK(same && at::localscan_own_hi(n, p.tile, l2) <= at::localscan_tile_end(0, p.tile, p.overlap, l2), "dropped tile %lld is not covered by tile 0", (long long)n);
		}
		const int64_t ns = at::localscan_swept(l2, p.tile, p.overlap), nfs = at::localscan_swept_full(l2, p.tile, p.overlap);
		CHECK(ns == p.ntiles - d && nfs >= 0 && nfs <= ns, "swept=%lld full=%lld", (long long)ns, (long long)nfs);
		for (int64_t k = 0; k < ns; ++k) {
			const int64_t n = at::localscan_swept_tile(k, d);
			CHECK(n < p.ntiles && (k == 0 ? n == 0 : n == k + d), "swept tile %lld is tile %lld", (long long)k, (long long)n);
			CHECK((n < p.nfull) == (k < nfs), "swept tile %lld (tile %lld): full=%d, among the first %lld", (long long)k, (long long)n, (int)(n < p.nfull), (long long)nfs);
		}
	}
	for (int q = 0; q < 4 && l2 > 0; ++q) {
		const int32_t ei = (int32_t)between(1, l1), score = (int32_t)between(0, mx * ei);
		const int64_t js = between(1, l2);
		const int64_t ws = at::localscan_window_start(js, ei, score, s.m, s.u, s.o, s.e);
		const int64_t sc1 = score > 1 ? score : 1;
		const int64_t gi = mx * ei - sc1 > 0 ? (mx * ei - sc1) / pen : 0;
		const int64_t want = js - ei - gi - ((-s.o) + (-s.e) - 1) / (-s.e) - 1;
		CHECK(ws % 16 == 0 && ws >= 0 && ws <= js, "ws=%lld j*=%lld", (long long)ws, (long long)js);
		CHECK(want <= 0 ? ws == 0 : (ws <= want && want - ws < 16), "ws=%lld want=%lld", (long long)ws, (long long)want);
	}
}

int main()
{
	const Sc scs[] = {{2, -2, -5, -2}, {1, -2, -5, -1}, {5, -4, -10, -1}, {3, -1, -1, -3}, {1, 3, -1, -1}, {7, -7, -3, -9}};
	const int32_t widths[] = {0, 16, 32, 48, 256, 1024, 4096};
	const int32_t cutoffs[] = {-3, 0, 1, 3, 40, 300, 5000};
	/* tile counts at the edges */
	for (int32_t T : {16, 48, 256, 2048}) {
		const int32_t l2s[] = {0, 1, T, T + 1, 64 * T, 64 * T + 1};
		const int64_t want[] = {0, 1, 1, 2, 64, 65};
		for (int x = 0; x < 6; ++x) {
			at::LocalScanPlan p;
			CHECK(at::localscan_plan(150, l2s[x], 0, 0, T, 2, -2, -5, -2, &p) == AT_OK && p.ntiles == want[x], "T=%d l2=%d tiles=%lld", T, l2s[x], (long long)p.ntiles);
			for (int32_t l1 : {1, 20, 1024})
				for (int uc = 0; uc < 2; ++uc) check_one(l1, l2s[x], uc, 12, T, scs[x % 6], true);
		}
		at::LocalScanPlan p;
		CHECK(at::localscan_plan(150, INT32_MAX, 0, 0, T, 2, -2, -5, -2, &p) == AT_OK && p.ntiles == ((int64_t)INT32_MAX + T - 1) / T, "T=%d l2=INT32_MAX", T);
		/* the last tiles of the longest target */
		for (int64_t n = p.ntiles - 3; n < p.ntiles; ++n) {
			const int64_t s0 = at::localscan_tile_start(n, p.tile, p.overlap), e = at::localscan_tile_end(n, p.tile, p.overlap, INT32_MAX);
			CHECK(s0 >= 0 && s0 % 16 == 0 && e > s0 && e <= INT32_MAX && e >= at::localscan_own_hi(n, p.tile, INT32_MAX), "tile %lld of INT32_MAX: (%lld, %lld]", (long long)n, (long long)s0, (long long)e);
		}
		CHECK(at::localscan_tile_end(p.ntiles - 1, p.tile, p.overlap, INT32_MAX) == INT32_MAX, "the last tile ends in l2");
	}
	for (int n = 0; n < 4000; ++n) {
		const Sc s = scs[rnd() % 6];
		const int32_t l1 = (int32_t)between(1, 1024);
		const bool big = n % 50 == 0;
		const int32_t l2 = big ? (int32_t)between(2000000000, 2147483647) : (int32_t)between(0, 100000);
		const int32_t T = big ? 4096 * 16 : widths[rnd() % 7];
		check_one(l1, l2, (int)(rnd() & 1), cutoffs[rnd() % 7], T, s, !big || n % 500 == 0);
	}
	/* l1 = 1 024 with m = 1 023: the largest product the key takes (1 023 * 1 024 < 2^20), overlap past 2^20, nothing wraps */
	{
		at::LocalScanPlan p;
		CHECK(at::localscan_plan(1024, INT32_MAX, 0, 0, 0, 1023, -1, -1, -1, &p) == AT_OK, "l1=1024 m=1023 refused");
		CHECK(p.overlap == ((1024 + (1023LL * 1024 - 1) + 15) & ~15LL), "overlap=%d", p.overlap);
		const int64_t last = p.ntiles - 1;
		CHECK(at::localscan_tile_start(last, p.tile, p.overlap) == last * p.tile - p.overlap && at::localscan_tile_end(last, p.tile, p.overlap, INT32_MAX) == INT32_MAX, "last tile");
		CHECK(at::localscan_plan(1024, 100, 0, 0, 0, 1024, -1, -1, -1, &p) == AT_ERR_DOMAIN, "m * l1 = 2^20 accepted");
		CHECK(at::localscan_plan(1024, 100, 0, 0, 0, 1, 1024, -1, -1, &p) == AT_ERR_DOMAIN, "u * l1 = 2^20 accepted");
		const int32_t top = 1023 * 1024;
		const unsigned long long k = at::localscan_key(top, 1024, INT32_MAX);
		CHECK(at::localscan_key_score(k) == top && at::localscan_key_end_i(k) == 1024 && at::localscan_key_end_j(k) == INT32_MAX, "key parts");
		CHECK(at::localscan_key(5, 3, 9) < at::localscan_key(4, 1, 1) && at::localscan_key(5, 3, 9) < at::localscan_key(5, 4, 1) &&
		      at::localscan_key(5, 3, 9) < at::localscan_key(5, 3, 10) && at::localscan_key(0, 1, 1) < ~0ull, "key order");
		CHECK(at::localscan_window_start(INT32_MAX, 1024, 1, 1023, -1, -1, -1) >= 0, "window at the top");
	}
	at::LocalScanPlan p;
	for (int32_t bad : {24, 8, -16, 1000, 17}) CHECK(at::localscan_plan(10, 100, 0, 0, bad, 2, -2, -5, -2, &p) == AT_ERR_ARG, "tile_cols=%d accepted", bad);
	CHECK(at::localscan_plan(-1, 100, 0, 0, 16, 2, -2, -5, -2, &p) == AT_ERR_ARG && at::localscan_plan(1, -100, 0, 0, 16, 2, -2, -5, -2, &p) == AT_ERR_ARG, "negative length accepted");
	CHECK(at::localscan_plan(10, 100, 0, 0, 16, 0, -2, -5, -2, &p) == AT_ERR_DOMAIN, "m = 0 accepted");
	CHECK(at::localscan_plan(10, 100, 0, 0, 16, 2, -2, 0, -2, &p) == AT_ERR_DOMAIN, "o = 0 accepted");
	CHECK(at::localscan_plan(10, 100, 0, 0, 16, 2, -2, -5, 0, &p) == AT_ERR_DOMAIN, "e = 0 accepted");
	CHECK(at::localscan_plan(10, 100, 0, 0, 16, 2, -2, -5, 1, &p) == AT_ERR_DOMAIN, "e = 1 accepted");
	CHECK(at::localscan_plan(0, 100, 0, 0, 16, 2, -2, -5, -2, &p) == AT_ERR_DOMAIN, "an empty query accepted");
	CHECK(at::localscan_plan(1025, 100, 0, 0, 16, 2, -2, -5, -2, &p) == AT_ERR_DOMAIN, "a 1 025-base query accepted");
	CHECK(at::localscan_plan(1024, 100, 0, 0, 16, 2, 7, -5, -2, &p) == AT_OK, "u > m refused");
	if (g_failures) { printf("localscan_plan_check: %d failures\n", g_failures); return 1; }
	printf("localscan_plan_check: ok\n");
	return 0;
}
