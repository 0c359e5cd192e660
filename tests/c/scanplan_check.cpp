/*
 * scanplan_check.cpp -- the scan planner (csrc/at_scanplan.h) without a GPU.  Built by `make asan` with AddressSanitizer and UBSan
 * and run by tests/test_scan_plan_check.py.  Over seeded (l1, l2, cutoff, tile_cols):
 *   1. the width is the caller's or the default, the overlap is the first multiple of 16 that holds l1 + c, the groups are
 *      ceil(l2 / (64 T)) and at least one; a width that is no multiple of 16 is AT_ERR_ARG;
 *   2. the own ranges of the lane-tiles cover the columns 1 .. l2 exactly once and in order, every sweep starts on a packed word,
 *      no further back than the overlap, and the tiles behind the target have no columns;
 *   3. a hit's window starts on a packed word, holds l1 + score columns in front of j* (or starts at 0) and is at most
 *      l1 + score + 15 columns wide.
 * Exit status 0 and "scanplan_check: ok" when everything holds; every failure is printed.
 */
#include "../../aligntools/c_amd/csrc/at_scanplan.h"

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

static void check_one(int32_t l1, int32_t l2, int use_cutoff, int32_t cutoff, int32_t tile_cols)
{
	at::ScanPlan p;
	const int rc = at::scan_plan(l1, l2, use_cutoff, cutoff, tile_cols, &p);
	CHECK(rc == AT_OK, "l1=%d l2=%d tile_cols=%d", l1, l2, tile_cols);
	if (rc != AT_OK) return;
	const int32_t c = !use_cutoff ? l1 : cutoff < 0 ? 0 : cutoff < l1 ? cutoff : l1;
	CHECK(p.tile == (tile_cols ? tile_cols : at::kScanDefaultTile) && p.tile % 16 == 0 && p.tile > 0, "tile=%d", p.tile);
	CHECK(p.overlap % 16 == 0 && p.overlap >= l1 + c && p.overlap < l1 + c + 16, "l1=%d c=%d overlap=%d", l1, c, p.overlap);
	const int64_t per = 64LL * p.tile;
	CHECK(p.ngroups == (l2 == 0 ? 1 : ((int64_t)l2 + per - 1) / per), "l2=%d tile=%d groups=%lld", l2, p.tile, (long long)p.ngroups);
	int64_t at_col = 0;
	for (int64_t n = 0; n < 64 * p.ngroups; ++n) {
		const int64_t s0 = at::scan_tile_start(n, p.tile, p.overlap), e = at::scan_tile_end(n, p.tile, l2);
		if (n * p.tile >= l2) { CHECK(e <= n * p.tile, "tile %lld behind the target has columns", (long long)n); continue; }
		CHECK(n * p.tile == at_col && e > at_col, "tile %lld owns (%lld, %lld], expected from %lld", (long long)n, (long long)(n * p.tile), (long long)e, (long long)at_col);
		CHECK(s0 % 16 == 0 && s0 >= 0 && s0 <= n * p.tile && (s0 == 0 || n * p.tile - s0 == p.overlap), "tile %lld sweeps from %lld", (long long)n, (long long)s0);
		at_col = e;
	}
	CHECK(at_col == l2, "covered %lld of %d", (long long)at_col, l2);
	for (int q = 0; q < 4; ++q) {
		const int32_t score = (int32_t)between(0, l1);
		const int64_t js = between(0, l2);
		const int64_t ws = at::scan_window_start(js, l1, score);
		CHECK(ws % 16 == 0 && ws >= 0 && ws <= js, "ws=%lld j*=%lld", (long long)ws, (long long)js);
		CHECK(ws == 0 || js - ws >= (int64_t)l1 + score, "window of %lld columns for l1=%d score=%d", (long long)(js - ws), l1, score);
		CHECK(js - ws <= (int64_t)l1 + score + 15 || ws == 0, "window of %lld columns for l1=%d score=%d", (long long)(js - ws), l1, score);
		CHECK(js - ws <= 2LL * l1 + 15 || (ws == 0 && js <= (int64_t)l1 + score), "window of %lld columns", (long long)(js - ws));
	}
}

int main()
{
	const int32_t widths[] = {0, 16, 32, 48, 256, 1024, 4096};
	const int32_t cutoffs[] = {-3, 0, 3, 12, 5000};
	for (int32_t T : {16, 48, 256, 1024})
		for (int32_t l2 : {0, 1, 64 * T - 1, 64 * T, 64 * T + 1})
			for (int32_t l1 : {0, 1, 1024})
				for (int uc = 0; uc < 2; ++uc) check_one(l1, l2, uc, 12, T);
	for (int n = 0; n < 4000; ++n) {
		const int32_t l1 = (int32_t)between(0, 1024);
		const int32_t l2 = n % 50 == 0 ? (int32_t)between(2000000000, 2147483647) : (int32_t)between(0, 300000);
		const int32_t T = l2 > 1000000 ? 4096 * 16 : widths[rnd() % 7];
		check_one(l1, l2, (int)(rnd() & 1), cutoffs[rnd() % 5], T);
	}
	at::ScanPlan p;
	for (int32_t bad : {24, 8, -16, 1000, 17}) CHECK(at::scan_plan(10, 100, 0, 0, bad, &p) == AT_ERR_ARG, "tile_cols=%d accepted", bad);
	CHECK(at::scan_plan(-1, 100, 0, 0, 16, &p) == AT_ERR_ARG && at::scan_plan(1, -100, 0, 0, 16, &p) == AT_ERR_ARG, "negative length accepted");
	if (g_failures) { printf("scanplan_check: %d failures\n", g_failures); return 1; }
	printf("scanplan_check: ok\n");
	return 0;
}
