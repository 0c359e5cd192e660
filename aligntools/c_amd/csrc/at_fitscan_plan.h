/*
 * at_fitscan_plan.h -- the plan of a fit scan (at_scan_fit): how a long target is cut into overlapping tiles that are
 * swept as ordinary fit pairs, and the window of the target in which a hit's alignment lies.  Pure arithmetic: plain C++17, no HIP.
 * The cut itself (tiles per target, the full shape, the tiles that repeat tile 0's sweep) is that of the local scan and is taken from
 * at_localscan_plan.h; what differs is the bound under which a path counts, the overlap, the window and the key.
 *
 * pen = min(|o|, |e|), mx = max(m, u).  Every candidate pair (l1 <= l2) scores at least lb = min(m, u) l1 + o + e: with l1 < l2 the
 * gapless diagonal that ends in column l1 is worth min(m, u) l1 at least; with l1 = l2 the end scan leaves the last column out, the
 * "+ o + e" stands for the gap row that closes a shorter diagonal, and the whole target is tile 0 anyway (ov > l1 = l2).  c = lb, or
 * max(cutoff, lb) with a cutoff.  g(l, s) = max(0, floor((mx l - s) / pen)) is the most gap columns a path over l rows can hold and still score >= s, so a
 * path that scores >= c spans at most l1 + g(l1, c) columns.  Tile n of a target OWNS the end columns n T <= j < (n + 1) T and is
 * swept as the fit pair (query, target columns (s0, e]) with s0 = max(0, n T - ov), ov = round16up(l1 + g(l1, c) + 1) and
 * e = min(l2, s0 + T + ov).  Fit's end scan leaves a pair's last column out: a tile's own last column is swept by the next tile, or
 * is the target's last column and left out in the full table too.  A tile's cells never exceed the full table's (row 0 is the full
 * table's, column 0 is -inf), so the lexicographic minimum of (-score, state is LOW, s0 + end_j) over the tiles is the exact
 * (score, state, j*) of every pair that scores >= c, and every other pair comes out below c.
 */
#pragma once
#include "at_localscan_plan.h"

namespace at {

constexpr int kFitScanDefaultTile = 1024;     /* own columns per tile when the caller names no width */
constexpr int kFitScanMaxQuery = 1024;
/* key = (SMAX - score) << 32 | (state is LOW) << 31 | absolute end_j: fit scores are negative as often as not, so the field is biased
 * over the whole int32 range but INT32_MIN (the sweeps' mark of a failed pair); no key of a result is all ones, the empty slot */
constexpr int64_t kFitScanSMax = INT32_MAX;
constexpr int64_t kFitScanScoreMin = -(int64_t)INT32_MAX;

struct FitScanPlan {
	int32_t tile;      /* T: own end columns per tile, a multiple of 16 */
	int32_t overlap;   /* ov: columns in front of the own range, a multiple of 16 */
	int64_t ntiles;    /* ceil(l2 / T); 0 for a target shorter than the query (no candidate) */
	int64_t nfull;     /* the tiles 0 .. nfull - 1 have exactly T + ov columns; the others end in column l2 and are shorter */
};

constexpr int fitscan_scoring_ok(int m, int o, int e) { return localscan_scoring_ok(m, o, e); }
constexpr int fitscan_query_ok(int32_t l1) { return l1 >= 1 && l1 <= kFitScanMaxQuery ? AT_OK : AT_ERR_DOMAIN; }

/* lb: every candidate pair scores at least this */
constexpr int64_t fitscan_floor(int32_t l1, int m, int u, int o, int e) { return (int64_t)(m < u ? m : u) * l1 + o + e; }

/* c */
constexpr int64_t fitscan_bound(int32_t l1, int use_cutoff, int32_t cutoff, int m, int u, int o, int e)
{
	const int64_t lb = fitscan_floor(l1, m, u, o, e);
	return use_cutoff && cutoff > lb ? cutoff : lb;
}

/* g(l, s): localscan_gap */
constexpr int64_t fitscan_gap(int64_t l, int64_t s, int m, int u, int o, int e) { return localscan_gap(l, s, m, u, o, e); }

/* ov; 64 bits: |u| is anything, so g has no bound an int32 keeps */
constexpr int64_t fitscan_overlap(int32_t l1, int use_cutoff, int32_t cutoff, int m, int u, int o, int e)
{
	return ((int64_t)l1 + fitscan_gap(l1, fitscan_bound(l1, use_cutoff, cutoff, m, u, o, e), m, u, o, e) + 1 + 15) & ~(int64_t)15;
}

/* a target shorter than the query is no candidate: no tiles */
constexpr int64_t fitscan_tiles(int32_t l1, int32_t l2, int32_t tile) { return l2 < l1 ? 0 : localscan_tiles(l2, tile); }
constexpr int64_t fitscan_full_tiles(int32_t l1, int32_t l2, int32_t tile, int64_t overlap) { return l2 < l1 ? 0 : localscan_full_tiles(l2, tile, overlap); }

/* tile n sweeps the target columns (start, end]; it owns the end columns own_lo <= j < own_hi (j < l2: the end scan's range) */
constexpr int64_t fitscan_tile_start(int64_t n, int32_t tile, int64_t overlap) { return localscan_tile_start(n, tile, overlap); }
constexpr int64_t fitscan_tile_end(int64_t n, int32_t tile, int64_t overlap, int32_t l2) { return localscan_tile_end(n, tile, overlap, l2); }
constexpr int64_t fitscan_own_lo(int64_t n, int32_t tile) { return n * tile; }
constexpr int64_t fitscan_own_hi(int64_t n, int32_t tile, int32_t l2) { return (n + 1) * tile < l2 ? (n + 1) * tile : l2; }

/* the tiles 1 .. d would repeat tile 0's sweep and are not swept; the swept tiles in order (localscan_dropped and its kin) */
constexpr int64_t fitscan_dropped(int32_t l1, int32_t l2, int32_t tile, int64_t overlap) { return l2 < l1 ? 0 : localscan_dropped(l2, tile, overlap); }
constexpr int64_t fitscan_swept_tile(int64_t k, int64_t d) { return localscan_swept_tile(k, d); }
constexpr int64_t fitscan_swept(int32_t l1, int32_t l2, int32_t tile, int64_t overlap) { return l2 < l1 ? 0 : localscan_swept(l2, tile, overlap); }
constexpr int64_t fitscan_swept_full(int32_t l1, int32_t l2, int32_t tile, int64_t overlap) { return l2 < l1 ? 0 : localscan_swept_full(l2, tile, overlap); }

/* AT_OK, AT_ERR_ARG for a negative length or a width that is negative or no multiple of 16, AT_ERR_DOMAIN for the scoring, the
 * query, or a tile that is no pair of the batch entry (int32 lengths) */
inline int fitscan_plan(int32_t l1, int32_t l2, int use_cutoff, int32_t cutoff, int32_t tile_cols, int m, int u, int o, int e, FitScanPlan *p)
{
	if (l1 < 0 || l2 < 0 || tile_cols < 0 || (tile_cols & 15)) return AT_ERR_ARG;
	if (fitscan_scoring_ok(m, o, e) != AT_OK || fitscan_query_ok(l1) != AT_OK) return AT_ERR_DOMAIN;
	const int64_t ov = fitscan_overlap(l1, use_cutoff, cutoff, m, u, o, e);
	p->tile = tile_cols > 0 ? tile_cols : kFitScanDefaultTile;
	if (ov + p->tile > INT32_MAX) return AT_ERR_DOMAIN;
	p->overlap = (int32_t)ov;
	p->ntiles = fitscan_tiles(l1, l2, p->tile);
	p->nfull = fitscan_full_tiles(l1, l2, p->tile, ov);
	return AT_OK;
}

/* the window (ws, we] of a hit that ends in (l1, j*) with this score: the fit pair (query, target columns (ws, we]) has the hit's
 * score and state, the end column j* - ws and the ops of the full table.  ws is a multiple of 16 (the window starts on a packed
 * word); we is one column past j* (the end scan leaves the last column out) and at least ws + l1 (fit refuses l1 > l2) */
constexpr int64_t fitscan_window_start(int64_t jstar, int32_t l1, int32_t score, int m, int u, int o, int e)
{
	const int64_t ae = localscan_abs(e), ao = localscan_abs(o);
	const int64_t x = jstar - l1 - fitscan_gap(l1, score, m, u, o, e) - (ao + ae - 1) / ae - 1;
	return x > 0 ? x & ~(int64_t)15 : 0;
}
constexpr int64_t fitscan_window_end(int64_t jstar, int64_t ws, int32_t l1, int32_t l2)
{
	const int64_t a = jstar + 1 > ws + l1 ? jstar + 1 : ws + l1;
	return a < l2 ? a : l2;
}

/* the key of a tile's result and its parts; fitscan_key_ok: the values fit their fields */
constexpr bool fitscan_key_ok(int64_t score, int64_t abs_j) { return score >= kFitScanScoreMin && score <= kFitScanSMax && abs_j >= 0 && abs_j <= INT32_MAX; }
constexpr unsigned long long fitscan_key(int32_t score, int low, int64_t abs_j)
{
	return ((unsigned long long)(kFitScanSMax - score) << 32) | ((unsigned long long)(low ? 1u : 0u) << 31) | (unsigned long long)((uint32_t)abs_j & 0x7fffffffu);
}
constexpr int32_t fitscan_key_score(unsigned long long key) { return (int32_t)(kFitScanSMax - (int64_t)(key >> 32)); }
constexpr int fitscan_key_low(unsigned long long key) { return (int)((key >> 31) & 1u); }
constexpr int32_t fitscan_key_end_j(unsigned long long key) { return (int32_t)((uint32_t)key & 0x7fffffffu); }

}  // namespace at
