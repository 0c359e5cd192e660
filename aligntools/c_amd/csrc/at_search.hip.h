/*
 * at_search.hip.h -- argument blocks and launches of the two kernels (at_search.hip) of a query-vs-target search (at_search,
 * include/aligntools_hip.h) around the unchanged sweeps.
 *
 * A search is cut into BLOCKS (one query-length group x the contiguous run of length-sorted targets it may meet) and every block
 * into SLICES of at most AT_ALLPAIRS_CHUNK pairs, ordered query-major: pair x of a block is (query qa + x / ntb, target ta + x % ntb)
 * in the sorted orders.  Per slice, on one stream:
 *   at_search_desc_k    writes the slice's woff1 / len1 / woff2 / len2 (24 bytes per pair), an ordinary descriptor batch for the sweep;
 *   (the sweep)         whatever align_device picks for the block's shape;
 *   at_search_merge_k   folds the slice's scores into per-query lists of the best K hits that stay in device memory.
 * A hit is a 64-bit key: the rank-ordered score in the high word (higher = better), the inverted caller index of the target in the
 * low word (smaller index = better), so one unsigned compare is the whole ranking rule and no two real keys are equal; 0 = empty.
 * The merged list is the top K of a total order over everything seen, so it does not depend on how the block was sliced.
 *
 * Strands (at_search_strands): with a reverse strand (`enc`) an entry of qperm is (caller query << 1) | strand, strand 1 being the
 * read nrev0 + query of the read set (its reverse complement, at_revcomp.hip), and the low word of a key is the inverted
 * (target << 1) | strand: after the target index, strand 0 ranks before strand 1.  With both strands (`two`) the two entries of a
 * query are adjacent in the block's order, strand 0 first, so the candidates of a caller query are still ONE contiguous run of
 * the block (2 ntb pairs) and one wavefront of the merge kernel owns the query's list, whichever strand a candidate is of.
 */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace at {

struct SearchDescArgs {
	long long s0, n;               /* the slice: block pairs [s0, s0 + n) */
	long long ntb;                 /* targets in the block */
	int qa, ta;                    /* the block's first query / target in the sorted orders */
	int nq;                        /* targets are reads nq .. of the read set */
	int enc;                       /* 0: qperm holds caller queries; 1: (query << 1) | strand */
	int nrev0;                     /* enc: the reverse complement of query q is read nrev0 + q */
	const int *qperm, *tperm;      /* sorted position -> caller index */
	const long long *swoff;        /* the read set's word offsets and lengths */
	const int *slen;
	long long *woff1, *woff2;      /* out: the slice's descriptors */
	int *len1, *len2;
};

struct SearchMergeArgs {
	long long s0, n, ntb;
	int qa, ta;
	int enc, two;                  /* enc as above; two: a caller query has two adjacent entries (both strands), else one */
	int nqs;                       /* caller queries with candidates in the slice; the first is s0 / (ntb << two) of the block */
	const int *qperm, *tperm;
	const int *score, *end_i, *end_j, *state;   /* the slice's results, indexed by pair - s0 */
	int k;                         /* 1 .. 64 */
	int is_edit, use_cutoff, cutoff;
	unsigned long long *lkey;      /* [nq * k] per caller query: keys in rank order (0 = empty) */
	int *lei, *lej, *lst;          /* [nq * k] the hits' end cells and states */
	int *bad;                      /* set to 1 if a candidate carries INT32_MIN */
};

}   // namespace at

/* at_search.hip: the launches (asynchronous on s; they return the launch's error) */
extern "C" hipError_t at_search_desc_launch(const at::SearchDescArgs *a, int ncu, hipStream_t s);
extern "C" hipError_t at_search_merge_launch(const at::SearchMergeArgs *a, hipStream_t s);
