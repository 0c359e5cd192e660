/*
 * at_pairhits.hip.h -- the selection stage of at_allpairs_hits (include/aligntools_hip.h; kernels in at_pairhits.hip).
 * All-vs-all over one read set, of which only the pairs over a threshold leave the device.  Per slice of n pairs, on the handle's
 * stream, behind the all-pairs sweep of the dense entries (align_device with ap_n > 0, unchanged) that left score / end_i / end_j /
 * state of every pair in four dense arrays:
 *   at_pairhits_flag_k   flag[p] = pair p is a hit: state != 0 (a pair with state 0 was proven below the threshold by the overlap
 *                        bound and holds that bound, not a score), score != INT32_MIN and score >= threshold (edit: distance <=
 *                        threshold).  The smallest pair index whose score is INT32_MIN (outside the reference's domain) is folded
 *                        into one 64-bit slot by atomicMin
 *   (at_scan_tiles / at_scan_nops of at_render.hip.h: the exclusive prefix sums of the flags)
 *   at_pairhits_emit_k   the kept pairs, in pair order, as PairHit records at their prefix sums (a, b from tri_pair of at_sweep.hip.h),
 *                        and the count next to the slot above: those 16 bytes and the kept records are all that crosses the link
 * and, for the alignments of the hits (pieces of at most 2^20 hits or 1 GB of op slots):
 *   at_pairhits_desc_k   hit records -> a pair list (woff1, len1, woff2, len2) and the op slots' sizes len[a] + len[b], whose prefix
 *                        sums are the slots' offsets; align_device sweeps the list with tracebacks, at_cigar_batch_device makes the runs
 *   at_pairhits_check_k  every pair's second-pass score and end cell equal the first pass's, else a flag word is set
 *
 * Out of scope: reverse-complement and swapped orientations (in all-pairs form the sweeps and the bound read both reads of a pair
 * from one per-read array), more than one GPU, CIGARs of edit distances, fit.
 */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace at {

struct PairHit {                   /* 32 bytes */
	long long pair;                /* the triangle index */
	int a, b;                      /* the reads, a < b */
	int score, end_i, end_j, state;
};

constexpr unsigned long long kPairHitsNoBad = ~0ull;

struct PairHitsArgs {
	long long n;                   /* pairs of the slice */
	long long first;               /* triangle index of the slice's pair 0 */
	long long nreads;
	const int *score, *end_i, *end_j, *state;   /* [n] the sweep's dense results */
	int threshold, is_edit;
	int *flag;                     /* [n] 0 / 1 */
	const long long *off;          /* [n + 1] prefix sums of flag */
	PairHit *hits;                 /* [cap] */
	long long cap;                 /* records the buffer holds (the slice's chunk: a slice always fits) */
	unsigned long long *slots;     /* [0] smallest pair index outside the domain (kPairHitsNoBad: none), [1] the kept count */
};

struct PairHitsDescArgs {
	long long n;                   /* hits of the piece */
	const PairHit *hits;
	const long long *swoff;        /* per read */
	const int *slen;
	long long *woff1, *woff2;      /* [n] */
	int *len1, *len2, *nslot;      /* [n]; nslot = len[a] + len[b] */
	/* the check: the second pass's results against the records */
	const int *score2, *end_i2, *end_j2;
	int *bad;
};

}   // namespace at

/* at_pairhits.hip (asynchronous on s; they return the launch's error) */
extern "C" hipError_t at_pairhits_flag_launch(const at::PairHitsArgs *a, int ncu, hipStream_t s);
extern "C" hipError_t at_pairhits_emit_launch(const at::PairHitsArgs *a, int ncu, hipStream_t s);
extern "C" hipError_t at_pairhits_desc_launch(const at::PairHitsDescArgs *a, int ncu, hipStream_t s);
extern "C" hipError_t at_pairhits_check_launch(const at::PairHitsDescArgs *a, int ncu, hipStream_t s);
