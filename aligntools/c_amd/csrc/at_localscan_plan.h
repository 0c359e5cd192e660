/*
 * at_localscan_plan.h -- the plan of a local scan (at_scan_local): how a long target is cut into overlapping tiles
 * that are swept as ordinary local pairs, and the window of the target in which a hit's alignment lies.  Pure arithmetic: plain
 * C++17, no HIP.
 *
 * pen = min(|o|, |e|), mx = max(m, u), c = max(1, cutoff) with a cutoff and 1 without.  g(l, s) = max(0, floor((mx l - s) / pen)) is the
 * most target-only gap columns a path over l rows can hold and still score >= s, so a path that scores >= c spans at most
 * l1 + g(l1, c) columns.  Tile n of a target OWNS the columns (n T, (n + 1) T] and is swept as the local pair (query, target columns
 * (s0, e]) with s0 = max(0, n T - ov), ov = round16up(l1 + g(l1, c)), and e = min(l2, s0 + T + ov): every tile but those at a
 * target's end has the one shape l1 x (T + ov), which is what the packed kernels ask for (the tiles that would repeat tile 0's
 * sweep are left out: localscan_dropped).  The columns behind the own range (only the
 * tiles with n T < ov have any) do no harm: a tile's cells never exceed the full table's, so whatever a tile reports is either
 * below the true maximum or a true maximum cell, and the lexicographic minimum of (-score, end_i, s0 + end_j) over the tiles is the
 * exact (score, i*, j*) of every pair that scores >= c.
 */
#pragma once
#include "../../../include/aligntools_hip.h"

#include <cstdint>

namespace at {

constexpr int kLocalScanDefaultTile = 1024;   /* own columns per tile when the caller names no width (DESIGN.md 3.15 has the runs) */
constexpr int kLocalScanMaxQuery = 1024;
constexpr int kLocalScanScoreBits = 20;       /* key = (SMAX - score) << 43 | end_i << 32 | absolute end_j */
constexpr int64_t kLocalScanSMax = (1LL << kLocalScanScoreBits) - 1;

struct LocalScanPlan {
	int32_t tile;      /* T: own columns per tile, a multiple of 16 */
	int32_t overlap;   /* ov: columns in front of the own range, a multiple of 16 */
	int64_t ntiles;    /* ceil(l2 / T) */
	int64_t nfull;     /* the tiles 0 .. nfull - 1 have exactly T + ov columns; the others end in column l2 and are shorter */
};

constexpr int64_t localscan_abs(int64_t x) { return x < 0 ? -x : x; }

/* AT_OK, or AT_ERR_DOMAIN for a scoring outside m >= 1, o <= -1, e <= -1 */
constexpr int localscan_scoring_ok(int m, int o, int e) { return m >= 1 && o <= -1 && e <= -1 ? AT_OK : AT_ERR_DOMAIN; }

constexpr int64_t localscan_mx(int m, int u) { return m > u ? m : u; }
constexpr int64_t localscan_pen(int o, int e) { return localscan_abs(o) < localscan_abs(e) ? localscan_abs(o) : localscan_abs(e); }

/* AT_OK, or AT_ERR_DOMAIN for a query outside 1 .. 1 024 bases or one whose best score would not fit the key */
constexpr int localscan_query_ok(int32_t l1, int m, int u)
{
	return l1 >= 1 && l1 <= kLocalScanMaxQuery && localscan_mx(m, u) * l1 < (1LL << kLocalScanScoreBits) ? AT_OK : AT_ERR_DOMAIN;
}

/* g(l, s) */
constexpr int64_t localscan_gap(int64_t l, int64_t s, int m, int u, int o, int e)
{
	const int64_t x = localscan_mx(m, u) * l - s;
	return x > 0 ? x / localscan_pen(o, e) : 0;
}

constexpr int64_t localscan_bound(int use_cutoff, int32_t cutoff) { return use_cutoff && cutoff > 1 ? cutoff : 1; }

/* ov; 64 bits: at l1 = 1 024, m = 1 023, pen = 1 it is past 2^20 */
constexpr int64_t localscan_overlap(int32_t l1, int use_cutoff, int32_t cutoff, int m, int u, int o, int e)
{
	return ((int64_t)l1 + localscan_gap(l1, localscan_bound(use_cutoff, cutoff), m, u, o, e) + 15) & ~(int64_t)15;
}

constexpr int64_t localscan_tiles(int32_t l2, int32_t tile) { return l2 <= 0 ? 0 : ((int64_t)l2 + tile - 1) / tile; }

/* first column a tile sweeps (exclusive: its columns are (s0, e]) and its last one */
constexpr int64_t localscan_tile_start(int64_t n, int32_t tile, int64_t overlap) { return n * tile - overlap > 0 ? n * tile - overlap : 0; }
constexpr int64_t localscan_tile_end(int64_t n, int32_t tile, int64_t overlap, int32_t l2)
{
	const int64_t e = localscan_tile_start(n, tile, overlap) + tile + overlap;
	return e < l2 ? e : l2;
}
/* the own range (lo, hi] of a tile */
constexpr int64_t localscan_own_lo(int64_t n, int32_t tile) { return n * tile; }
constexpr int64_t localscan_own_hi(int64_t n, int32_t tile, int32_t l2) { return (n + 1) * tile < l2 ? (n + 1) * tile : l2; }

/* the tiles with the full shape come first: a target shorter than T + ov has none, any other all but its last (all, if T divides l2) */
constexpr int64_t localscan_full_tiles(int32_t l2, int32_t tile, int64_t overlap)
{
	const int64_t n = localscan_tiles(l2, tile);
	return (int64_t)l2 < tile + overlap ? 0 : l2 % tile ? n - 1 : n;
}

/* The tiles 1 .. d with d T <= ov start in column 0 and end where tile 0 ends: they would repeat tile 0's sweep and are NOT swept (tile
 * 0's sweep covers their own columns).  The swept tiles in order are tile 0 and the tiles d + 1 .. : swept tile k is tile
 * localscan_swept_tile(k, d); the first localscan_swept_full of them have the full shape (tiles 0 .. d all have it, or none has). */
constexpr int64_t localscan_dropped(int32_t l2, int32_t tile, int64_t overlap)
{
	const int64_t n = localscan_tiles(l2, tile), d = overlap / tile;
	return n <= 0 ? 0 : d < n - 1 ? d : n - 1;
}
constexpr int64_t localscan_swept_tile(int64_t k, int64_t d) { return k == 0 ? 0 : k + d; }
constexpr int64_t localscan_swept(int32_t l2, int32_t tile, int64_t overlap) { return localscan_tiles(l2, tile) - localscan_dropped(l2, tile, overlap); }
constexpr int64_t localscan_swept_full(int32_t l2, int32_t tile, int64_t overlap)
{
	const int64_t nf = localscan_full_tiles(l2, tile, overlap);
	return nf > 0 ? nf - localscan_dropped(l2, tile, overlap) : 0;
}

/* AT_OK, AT_ERR_ARG for a negative length or a width that is negative or no multiple of 16, AT_ERR_DOMAIN for the scoring / query */
inline int localscan_plan(int32_t l1, int32_t l2, int use_cutoff, int32_t cutoff, int32_t tile_cols, int m, int u, int o, int e, LocalScanPlan *p)
{
	if (l1 < 0 || l2 < 0 || tile_cols < 0 || (tile_cols & 15)) return AT_ERR_ARG;
	if (localscan_scoring_ok(m, o, e) != AT_OK || localscan_query_ok(l1, m, u) != AT_OK) return AT_ERR_DOMAIN;
	const int64_t ov = localscan_overlap(l1, use_cutoff, cutoff, m, u, o, e);
	p->tile = tile_cols > 0 ? tile_cols : kLocalScanDefaultTile;
	if (ov + p->tile > INT32_MAX) return AT_ERR_DOMAIN;   /* (a tile is one pair of the batch entry: int32 lengths) */
	p->overlap = (int32_t)ov;
	p->ntiles = localscan_tiles(l2, p->tile);
	p->nfull = localscan_full_tiles(l2, p->tile, ov);
	return AT_OK;
}

/* ws of a hit that ends in (i*, j*) with this score: the pair (query, target columns (ws, j*]) has the hit's score, the end cell
 * (i*, j* - ws) and the ops of the full table; a multiple of 16, so the window starts on a packed word */
constexpr int64_t localscan_window_start(int64_t jstar, int32_t istar, int32_t score, int m, int u, int o, int e)
{
	const int64_t ae = localscan_abs(e), ao = localscan_abs(o);
	const int64_t x = jstar - istar - localscan_gap(istar, score > 1 ? score : 1, m, u, o, e) - (ao + ae - 1) / ae - 1;
	return x > 0 ? x & ~(int64_t)15 : 0;
}

/* the key of a tile's result and its parts */
constexpr unsigned long long localscan_key(int32_t score, int32_t end_i, int64_t abs_j)
{
	return ((unsigned long long)(kLocalScanSMax - score) << 43) | ((unsigned long long)(unsigned)end_i << 32) | (unsigned long long)(uint32_t)abs_j;
}
constexpr int32_t localscan_key_score(unsigned long long key) { return (int32_t)(kLocalScanSMax - (int64_t)(key >> 43)); }
constexpr int32_t localscan_key_end_i(unsigned long long key) { return (int32_t)((key >> 32) & 0x7ffu); }
constexpr int32_t localscan_key_end_j(unsigned long long key) { return (int32_t)(uint32_t)key; }

}  // namespace at
