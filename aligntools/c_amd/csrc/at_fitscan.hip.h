/*
 * at_fitscan.hip.h -- end-to-end affine alignment of reads against LONG targets (at_scan_fit, include/aligntools_hip.h; kernels in
 * at_fitscan.hip): the result of at_align_batch(AT_MODE_FIT), use_jump off, for every (query or its reverse complement, target no
 * shorter than the query) with no bound on the target length.  DESIGN.md 3.18 has the two facts behind it and their argument;
 * at_fitscan_plan.h the arithmetic.
 *
 * The sweep is not written here: a tile is an ordinary fit pair (query, target columns (s0, e]) and goes through the batch entry
 * (align_device), scores only.  The targets are sorted by length as in at_search: a block is the entries of one query length x the
 * targets no shorter than it (tperm[ta ..]).  A work item is (query entry, target, tile); item y of a block is (entry y / A, target,
 * tile) with A the tiles of the block's targets and the target found by bisection in a prefix array of tiles per target.  The tiles
 * of the one shape l1 x (T + ov) and the shorter ones at the targets' ends are two passes with a prefix array each, so the first is a
 * uniform batch.  Per slice of at most AT_ALLPAIRS_CHUNK tile pairs:
 *   at_fitscan_desc_k     item -> woff1 / len1 / woff2 = the target's words + s0 / bases per word / len2 = e - s0
 *   (align_device)
 *   at_fitscan_fold_k     one thread per tile pair: key = (SMAX - score) << 32 | (state is LOW) << 31 | s0 + end_j, one 64-bit
 *                         atomicMin into the slot of (query entry, target); a value outside its field or a failed pair raises the flag
 *                         word of the search
 * The slots of a run of pairs (at_localscan_init_k, unchanged: all ones) stay until every tile of the run is folded; then
 *   at_fitscan_unpack_k   slot -> score / end_i = l1 / end_j / state for at_search_merge_k, unchanged
 * and for the alignments of the hits, over the USED list entries (the host names them), in pieces:
 *   at_fitscan_window_k   window pairs: the query (or its reverse complement) against target columns (ws, we]
 *   (align_device with tracebacks and the CIGAR kernels, unchanged)
 *   at_fitscan_check_k    the window's score, state and end column must reproduce the hit (a flag word otherwise); AT_CG_START_J += ws
 * Every store is checked against the capacity the host names.
 */
#pragma once
#include <hip/hip_runtime.h>
#include "at_fitscan_plan.h"

namespace at {

struct FitScanArgs {
	long long y0, nitems;          /* the slice's items: [y0, y0 + nitems) of the pass; its stores go to [0, cap) */
	long long cap;
	long long p0, npairs;          /* the run's pairs: [p0, p0 + npairs) of the block, pair x = (entry qa + x / ntb, target tperm[ta + x % ntb]) */
	long long ntb, tall;           /* the block's targets; items of all of them together in this pass */
	const long long *tpre;         /* [ntb + 1] items of the block's targets in front of its target t in this pass */
	int ragged;                    /* the pass: 0 = the full-shape tiles of a target, 1 = the shorter ones behind them */
	int qa, ta, nq;                /* the block's first entry of qperm and first target of tperm; targets are reads nq .. of the read set */
	int enc, nrev0;                /* as SearchDescArgs */
	int bpw;                       /* bases per packed word: 16 or 4 */
	const int *qperm, *tperm;
	const long long *swoff;
	const int *slen;
	int tile;
	long long overlap;
	long long *woff1, *woff2;      /* at_fitscan_desc_k: [cap] */
	int *len1, *len2;
	long long *s0;                 /* [cap] the tile's first column */
	long long *slot;               /* [cap] the tile's pair of the run */
	const int *score, *end_j, *state;   /* at_fitscan_fold_k: what the sweep found, [cap] */
	unsigned long long *key;       /* [npairs] */
	int *bad;
	int *o_score, *o_end_i, *o_end_j, *o_state;   /* at_fitscan_unpack_k: [npairs] */
};

struct FitScanWindowArgs {
	long long n;                   /* the piece's hits; everything below marked [n] is indexed by the hit's place in the piece */
	long long nlist;               /* list entries: nq * k */
	const long long *eidx;         /* [n] the list entry of each hit: used entries only, ascending */
	int k, nq, enc, nrev0, bpw;
	int m, u, o, e;
	const unsigned long long *lkey;   /* the lists of at_search_merge_k */
	const int *lej, *lst;
	const long long *swoff;
	const int *slen;
	long long *woff1, *woff2;      /* out: the window pairs [n] */
	int *len1, *len2, *ws;
	/* at_fitscan_check_k */
	const int *w_score, *w_end_j, *w_state;   /* what the traceback pass found in the windows [n] */
	const int *ncigar;             /* [n] */
	int *stats;                    /* [n][8] */
	int *bad;
};

}   // namespace at

/* at_fitscan.hip: the launches (asynchronous on s; they return the launch's error) */
extern "C" hipError_t at_fitscan_desc_launch(const at::FitScanArgs *a, int ncu, hipStream_t s);
extern "C" hipError_t at_fitscan_fold_launch(const at::FitScanArgs *a, int ncu, hipStream_t s);
extern "C" hipError_t at_fitscan_unpack_launch(const at::FitScanArgs *a, int ncu, hipStream_t s);
extern "C" hipError_t at_fitscan_window_launch(const at::FitScanWindowArgs *a, int ncu, hipStream_t s);
extern "C" hipError_t at_fitscan_check_launch(const at::FitScanWindowArgs *a, int ncu, hipStream_t s);
