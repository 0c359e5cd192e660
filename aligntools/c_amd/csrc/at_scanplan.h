/*
 * at_scanplan.h -- the plan of a scan (at_scan): how a long target is cut into overlapping tiles that are swept
 * independently, and the window of the target in which a hit's alignment lies.  Pure arithmetic: plain C++17, no HIP.
 *
 * Lane-tile n of a target owns the columns (n T, (n + 1) T] and starts its sweep at s0 = max(0, n T - ov), treating s0 as column 0;
 * ov = round16up(l1 + c), c = l1 without a cutoff, min(l1, cutoff) with one.  An alignment that ends in column j consumes at most
 * l1 + D(l1,j) target columns, so every own column whose D is <= c comes out exact and every other one too high: the lexicographic
 * minimum of (score, column) over the tiles and the candidate (l1, 0) is the exact (score, j*) of every pair that scores <= c.
 * 64 consecutive tiles (one per lane) are a GROUP, the work item of one wavefront.
 */
#pragma once
#include "../../../include/aligntools_hip.h"

#include <cstdint>

namespace at {

constexpr int kScanDefaultTile = 2048;   /* columns a lane owns when the caller names no width (DESIGN.md 3.12 has the runs) */
constexpr int kScanMaxQuery = 1024;      /* the longest read of the bit-parallel lane kernels */

struct ScanPlan {
	int32_t tile;      /* T: own columns per lane, a multiple of 16 */
	int32_t overlap;   /* ov: warm-up columns in front of a tile, a multiple of 16 */
	int64_t ngroups;   /* ceil(l2 / (64 T)), at least 1 */
};

/* c of the header: the largest score that must come out exact */
constexpr int32_t scan_exact_bound(int32_t l1, int use_cutoff, int32_t cutoff)
{
	return !use_cutoff || cutoff >= l1 ? l1 : cutoff < 0 ? 0 : cutoff;
}

constexpr int32_t scan_overlap(int32_t l1, int use_cutoff, int32_t cutoff)
{
	return (int32_t)(((int64_t)l1 + scan_exact_bound(l1, use_cutoff, cutoff) + 15) & ~(int64_t)15);
}

constexpr int64_t scan_groups(int32_t l2, int32_t tile)
{
	const int64_t per = 64LL * tile;
	return l2 <= 0 ? 1 : ((int64_t)l2 + per - 1) / per;
}

/* AT_OK, or AT_ERR_ARG for a negative length or a width that is negative or no multiple of 16 */
inline int scan_plan(int32_t l1, int32_t l2, int use_cutoff, int32_t cutoff, int32_t tile_cols, ScanPlan *p)
{
	if (l1 < 0 || l2 < 0 || tile_cols < 0 || (tile_cols & 15)) return AT_ERR_ARG;
	p->tile = tile_cols > 0 ? tile_cols : kScanDefaultTile;
	p->overlap = scan_overlap(l1, use_cutoff, cutoff);
	p->ngroups = scan_groups(l2, p->tile);
	return AT_OK;
}

/* first column a lane-tile sweeps (exclusive: its columns are (s0, e]) and its last one; e <= s0: the tile lies behind the target */
constexpr int64_t scan_tile_start(int64_t n, int32_t tile, int32_t overlap) { return n * tile - overlap > 0 ? n * tile - overlap : 0; }
constexpr int64_t scan_tile_end(int64_t n, int32_t tile, int32_t l2) { return (n + 1) * tile < l2 ? (n + 1) * tile : l2; }

/* ws of a hit: the pair (read, target columns (ws, j*]) has the hit's score, its end column is j* - ws and its ops are those of
 * the full table; a multiple of 16, so the window starts on a packed word */
constexpr int64_t scan_window_start(int64_t jstar, int32_t l1, int32_t score)
{
	return jstar - l1 - score > 0 ? (jstar - l1 - score) & ~(int64_t)15 : 0;
}

}  // namespace at
