/*
 * at_tilescan.hip.h -- reads against LONG targets, cut into tiles: the kernels around the sweep of at_scan_local (Smith-Waterman,
 * DESIGN.md 3.15) and of at_scan_fit (end-to-end affine alignment, 3.18), include/aligntools_hip.h; kernels in at_tilescan.hip.  Both
 * give the result of at_align_batch in their mode for every (query or its reverse complement, target) with no bound on the target
 * length; the two sections have the facts behind that and their proofs, at_localscan_plan.h and at_fitscan_plan.h the arithmetic.
 *
 * The sweep is not written here: a tile is an ordinary pair of the mode (query, target columns (s0, e]) and goes through the batch
 * entry (align_device), scores only.  A block is the entries of one query length x its targets tperm[ta .. ta + ntb): all targets in
 * caller order for local, the targets no shorter than the queries, sorted by length as in at_search, for fit.  A work item is (query
 * entry, target, tile); item y of a block is (entry y / A, target, tile) with A the tiles of the block's targets and the target found
 * by bisection in a prefix array of tiles per target.  The tiles of the one shape l1 x (T + ov) and the shorter ones at the targets'
 * ends are two passes with a prefix array each, so the first is a uniform batch.  Per slice of at most AT_ALLPAIRS_CHUNK tile pairs:
 *   at_tilescan_desc_k     item -> woff1 / len1 / woff2 = the target's words + s0 / bases per word / len2 = e - s0
 *   (align_device)
 *   at_tilescan_fold_k     one thread per tile pair: one 64-bit atomicMin of the tile's key into the slot of (query entry, target); a
 *                          value outside its field or a failed pair raises the flag word of the search
 * The slots of a run of pairs (at_tilescan_init_k: all ones) stay until every tile of the run is folded; then
 *   at_tilescan_unpack_k   slot -> score / end_i / end_j / state for at_search_merge_k, unchanged
 * and for the alignments of the hits, over the USED list entries (the host names them), in pieces:
 *   at_tilescan_window_k   window pairs: the query (or its reverse complement) against the target columns of the hit's window
 *   (align_device with tracebacks and the CIGAR kernels, unchanged)
 *   at_tilescan_check_k    the window must reproduce the hit (a flag word otherwise); AT_CG_START_J += ws
 * Unused entries never reach the device: the host leaves them 0 runs and a statistics row of -1.
 * Every store is checked against the capacity the host names.
 *
 * What the two families do differently (a template parameter of the kernels, the mode of the launches) is the table of DESIGN.md 3.15.
 */
#pragma once
#include <hip/hip_runtime.h>
#include "at_fitscan_plan.h"

namespace at {

struct TileScanArgs {
	long long y0, nitems;          /* the slice's items: [y0, y0 + nitems) of the pass; its stores go to [0, cap) */
	long long cap;
	long long p0, npairs;          /* the run's pairs: [p0, p0 + npairs) of the block, pair x = (entry qa + x / ntb, target tperm[ta + x % ntb]) */
	long long ntb, tall;           /* the block's targets; items of all of them together in this pass.  A FIT block must hold no target
	                                * shorter than its queries (the host's block filter): the kernels cut every target as local does */
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
	long long *woff1, *woff2;      /* at_tilescan_desc_k: [cap] */
	int *len1, *len2;
	long long *s0;                 /* [cap] the tile's first column */
	long long *slot;               /* [cap] the tile's pair of the run */
	const int *score, *end_i, *end_j, *state;   /* at_tilescan_fold_k: what the sweep found, [cap] (local reads end_i, fit state) */
	unsigned long long *key;       /* [npairs] */
	int *bad;
	int *o_score, *o_end_i, *o_end_j, *o_state;   /* at_tilescan_unpack_k: [npairs] */
};

struct TileScanWindowArgs {
	long long n;                   /* the piece's hits; everything below marked [n] is indexed by the hit's place in the piece */
	long long nlist;               /* list entries: nq * k */
	const long long *eidx;         /* [n] the list entry of each hit: used entries only, ascending */
	int k, nq, enc, nrev0, bpw;
	int m, u, o, e;
	const unsigned long long *lkey;   /* the lists of at_search_merge_k */
	const int *lei, *lej, *lst;
	const long long *swoff;
	const int *slen;
	long long *woff1, *woff2;      /* out: the window pairs [n] */
	int *len1, *len2, *ws;
	/* at_tilescan_check_k */
	const int *w_score, *w_end_i, *w_end_j, *w_state;   /* what the traceback pass found in the windows [n] */
	const int *ncigar;             /* [n] */
	int *stats;                    /* [n][8] */
	int *bad;
};

}   // namespace at

/* at_tilescan.hip: the launches (asynchronous on s; they return the launch's error); mode: AT_MODE_LOCAL or AT_MODE_FIT */
extern "C" hipError_t at_tilescan_desc_launch(int mode, const at::TileScanArgs *a, int ncu, hipStream_t s);
extern "C" hipError_t at_tilescan_init_launch(const at::TileScanArgs *a, int ncu, hipStream_t s);
extern "C" hipError_t at_tilescan_fold_launch(int mode, const at::TileScanArgs *a, int ncu, hipStream_t s);
extern "C" hipError_t at_tilescan_unpack_launch(int mode, const at::TileScanArgs *a, int ncu, hipStream_t s);
extern "C" hipError_t at_tilescan_window_launch(int mode, const at::TileScanWindowArgs *a, int ncu, hipStream_t s);
extern "C" hipError_t at_tilescan_check_launch(int mode, const at::TileScanWindowArgs *a, int ncu, hipStream_t s);
