/*
 * at_scan.hip.h -- reads against LONG targets (at_scan, include/aligntools_hip.h; kernels in at_scan.hip): the rule of edit infix mode
 * (at_infix.hip.h) with no bound on the target length.  DESIGN.md 3.12 has the two facts behind it and their proofs.
 *
 * A target is cut into lane-tiles of T own columns with ov warm-up columns in front (at_scanplan.h); 64 consecutive tiles are a
 * GROUP.  A work item is (query entry, target, group): ONE READ PER WAVEFRONT, its 64 lanes sweep the same read against 64
 * consecutive tiles of one target.
 *   - l1, the pad and the read's bit planes B0 / B1 / pad are wave-uniform: they are formed through readfirstlane and live in SGPRs
 *     (a VALU instruction takes one SGPR operand: B0 ^ nC0, B1 ^ nC1 and each v_or3 have exactly one).  At 32 words the three
 *     planes would need 96 SGPRs: there the pad words stay in VGPRs.  Pv / Mv and the column's code are per lane.
 *   - no LDS: a lane needs one packed target word per sixteen columns and loads it from global memory one word ahead; the lanes
 *     read T / 16 words apart.  Occupancy is bounded by registers alone and l2 by nothing.
 *   - the word step is that of at_infix.hip (bottom-aligned rows, wildcard pad rows), repeated once more for the reason given there.
 *   - the lanes step together for the longest tile of the group; a lane keeps best / best_j under a strict < while inside its own
 *     tile, starting from (l1, s0).  Warm-up columns are not masked: they only ever over-estimate.
 *   - at the end the wave takes the minimum of ((uint64)best << 32) | absolute best_j across its lanes and one lane folds it with a
 *     64-bit atomicMin into the slot of its pair, which at_scan_init_k set to (l1 << 32) | 0, the candidate (l1, 0).
 * Items come from the device queue (next_work).  Item y of a block is (query entry y / G, target, group) with G the groups of all
 * targets and the target found by bisection in the prefix array of groups per target.
 *
 * Around the sweep, per slice of pairs (the blocks and slices of at_search.hip.h with the targets in caller order):
 *   at_scan_init_k     the slice's key slots
 *   at_scan<W>         the groups of the slice's pairs
 *   at_scan_unpack_k   key -> score / end_i / end_j / state, the input of at_search_merge_k (same total order, same lists)
 * and for the alignments of the hits, over the nq * k list entries:
 *   at_scan_window_k   window descriptors: the read (or its reverse complement) against target columns (ws, j*], ws a multiple of 16
 *   (at_infix<W, true> and the CIGAR kernels, unchanged)
 *   at_scan_check_k    the window's score and end column must reproduce the hit (a flag word otherwise); AT_CG_START_J += ws;
 *                      unused entries: 0 runs and a statistics row of -1
 *
 * at_scan<W, true> (at_scan_hits) is the same sweep without best / best_j, shuffles and slot: per column a lane asks
 * whether the sign pair says -1, d <= c and the column is an OWN column (warm-up columns never count here: a tile sees exactly the
 * descents of its own columns), keeps the run of such descents in consecutive columns (first value, latest value) and, in the first
 * column behind a run, appends ONE record to the slice's candidate buffer: an atomicAdd on the slice's counter, which counts on past
 * the capacity, and the stores only while the index is below it.  The block with the atomic and the stores is skipped by the wave
 * when no lane has a record.  Behind the sweep: sort, marking, compaction (at_scanhits.hip.h); the window kernels serve the kept hits
 * with the query of each entry in `eq` and END-ANCHORED windows (InfixArgs::anchor_end).
 */
#pragma once
#include "at_myers.hip.h"
#include "at_scanplan.h"
#include "at_scanhits.h"

namespace at {

struct ScanArgs {
	long long y0, nitems;          /* the slice's items: [y0, y0 + nitems) of the block */
	long long s0, npairs;          /* the slice's pairs: [s0, s0 + npairs) of the block, pair x = (entry qa + x / ntb, target x % ntb) */
	long long ntb, gall;           /* targets; groups of all targets together */
	const long long *gpre;         /* [ntb + 1] groups of the targets in front of target t */
	int qa, nq;                    /* the block's first entry of qperm; targets are reads nq .. of the read set */
	int enc, nrev0;                /* as SearchDescArgs */
	const int *qperm;
	const uint32_t *seq;           /* the read set: 2-bit packed words, word offsets, lengths */
	const long long *swoff;
	const int *slen;
	int tile, use_cutoff, cutoff;
	unsigned long long *key;       /* [npairs] */
	unsigned long long *queue;
	int *score, *end_i, *end_j, *state;   /* at_scan_unpack_k: [npairs] */
	/* at_scan<W, true>: the slice's candidate records (at_scanhits.h), key = (pair of the slice << 32) | last column of a run of
	 * descents, val = its last and first value; *cand_n counts every record, stored or not: one is stored only while its index is
	 * below cand_cap */
	unsigned long long *cand_n;
	long long cand_cap;
	unsigned long long *cand_key;
	int *cand_val;
};

struct ScanWindowArgs {
	long long n;                   /* list entries: nq * k */
	int k, nq, enc, nrev0;
	const unsigned long long *lkey;   /* the lists of at_search_merge_k */
	const int *lej;
	const int *eq;                 /* the query of entry e, or NULL: e / k */
	const long long *swoff;
	const int *slen;
	long long *woff1, *woff2;      /* out: the window pairs */
	int *len1, *len2, *ws;
	/* at_scan_check_k */
	const int *w_score, *w_end_j;  /* what at_infix<W, true> found in the windows */
	const int *ncigar;
	int *stats;                    /* [n][8] */
	int *ncigar_out;
	int *bad;
};

}   // namespace at

/* at_scan.hip: the launches (asynchronous on s; they return the launch's error).  w: words per lane of kMyersLaneWords */
extern "C" const void *at_scan_kernel(int w);
extern "C" hipError_t at_scan_init_launch(const at::ScanArgs *a, int ncu, hipStream_t s);
extern "C" hipError_t at_scan_launch(const at::ScanArgs *a, int w, unsigned grid, hipStream_t s);
extern "C" const void *at_scan_hits_kernel(int w);
extern "C" hipError_t at_scan_hits_launch(const at::ScanArgs *a, int w, unsigned grid, hipStream_t s);
extern "C" hipError_t at_scan_unpack_launch(const at::ScanArgs *a, int ncu, hipStream_t s);
extern "C" hipError_t at_scan_window_launch(const at::ScanWindowArgs *a, int ncu, hipStream_t s);
extern "C" hipError_t at_scan_check_launch(const at::ScanWindowArgs *a, int ncu, hipStream_t s);
