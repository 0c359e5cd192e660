/*
 * at_localscan.hip.h -- Smith-Waterman of reads against LONG targets (at_scan_local, include/aligntools_hip.h; kernels in
 * at_localscan.hip): the result of at_align_batch(AT_MODE_LOCAL) for every (query or its reverse complement, target) with no bound
 * on the target length.  DESIGN.md 3.15 has the two facts behind it and their proofs; at_localscan_plan.h the arithmetic.
 *
 * The sweep is not written here: a tile is an ordinary local pair (query, target columns (s0, e]) and goes through the batch entry
 * (align_device), scores only.  A work item is (query entry, target, tile); item y of a block is (entry y / A, target, tile) with A
 * the tiles of all targets and the target found by bisection in a prefix array of tiles per target.  The tiles of the one shape
 * l1 x (T + ov) and the shorter ones at the targets' ends are two passes with a prefix array each, so the first is a uniform batch.
 * Per slice of at most AT_ALLPAIRS_CHUNK tile pairs:
 *   at_localscan_desc_k     item -> woff1 / len1 / woff2 = the target's words + s0 / bases per word / len2 = e - s0
 *   (align_device)
 *   at_localscan_fold_k     one thread per tile pair: key = (SMAX - score) << 43 | end_i << 32 | s0 + end_j, one 64-bit atomicMin into
 *                           the slot of (query entry, target); a pair outside the domain raises the flag word of the search
 * The slots of a run of pairs (at_localscan_init_k: all ones) stay until every tile of the run is folded; then
 *   at_localscan_unpack_k   slot -> score / end_i / end_j / state for at_search_merge_k, unchanged
 * and for the alignments of the hits, over the USED list entries (the host names them), in pieces:
 *   at_localscan_window_k   window pairs: the query (or its reverse complement) against target columns (ws, j*]
 *   (align_device with tracebacks and the CIGAR kernels, unchanged)
 *   at_localscan_check_k    the window's score and end cell must reproduce the hit (a flag word otherwise); AT_CG_START_J += ws
 * Unused entries never reach the device: the host leaves them 0 runs and a statistics row of -1.
 * Every store is checked against the capacity the host names.
 */
#pragma once
#include <hip/hip_runtime.h>
#include "at_localscan_plan.h"

namespace at {

struct LocalScanArgs {
	long long y0, nitems;          /* the slice's items: [y0, y0 + nitems) of the pass; its stores go to [0, cap) */
	long long cap;
	long long p0, npairs;          /* the run's pairs: [p0, p0 + npairs) of the block, pair x = (entry qa + x / ntb, target x % ntb) */
	long long ntb, tall;           /* targets; items of all targets together in this pass */
	const long long *tpre;         /* [ntb + 1] items of the targets in front of target t in this pass */
	int ragged;                    /* the pass: 0 = tiles 0 .. nfull - 1 of a target, 1 = tiles nfull .. */
	int qa, nq;                    /* the block's first entry of qperm; targets are reads nq .. of the read set */
	int enc, nrev0;                /* as SearchDescArgs */
	int bpw;                       /* bases per packed word: 16 or 4 */
	const int *qperm;
	const long long *swoff;
	const int *slen;
	int tile;
	long long overlap;
	long long *woff1, *woff2;      /* at_localscan_desc_k: [cap] */
	int *len1, *len2;
	long long *s0;                 /* [cap] the tile's first column */
	long long *slot;               /* [cap] the tile's pair of the run */
	const int *score, *end_i, *end_j;   /* at_localscan_fold_k: what the sweep found, [cap] */
	unsigned long long *key;       /* [npairs] */
	int *bad;
	int *o_score, *o_end_i, *o_end_j, *o_state;   /* at_localscan_unpack_k: [npairs] */
};

struct LocalScanWindowArgs {
	long long n;                   /* the piece's hits; everything below marked [n] is indexed by the hit's place in the piece */
	long long nlist;               /* list entries: nq * k */
	const long long *eidx;         /* [n] the list entry of each hit: used entries only, ascending */
	int k, nq, enc, nrev0, bpw;
	int m, u, o, e;
	const unsigned long long *lkey;   /* the lists of at_search_merge_k */
	const int *lei, *lej;
	const long long *swoff;
	const int *slen;
	long long *woff1, *woff2;      /* out: the window pairs [n] */
	int *len1, *len2, *ws;
	/* at_localscan_check_k */
	const int *w_score, *w_end_i, *w_end_j;   /* what the traceback pass found in the windows [n] */
	const int *ncigar;             /* [n] */
	int *stats;                    /* [n][8] */
	int *bad;
};

}   // namespace at

/* at_localscan.hip: the launches (asynchronous on s; they return the launch's error) */
extern "C" hipError_t at_localscan_desc_launch(const at::LocalScanArgs *a, int ncu, hipStream_t s);
extern "C" hipError_t at_localscan_init_launch(const at::LocalScanArgs *a, int ncu, hipStream_t s);
extern "C" hipError_t at_localscan_fold_launch(const at::LocalScanArgs *a, int ncu, hipStream_t s);
extern "C" hipError_t at_localscan_unpack_launch(const at::LocalScanArgs *a, int ncu, hipStream_t s);
extern "C" hipError_t at_localscan_window_launch(const at::LocalScanWindowArgs *a, int ncu, hipStream_t s);
extern "C" hipError_t at_localscan_check_launch(const at::LocalScanWindowArgs *a, int ncu, hipStream_t s);
