/*
 * at_scanhits.hip.h -- the selection stage of at_scan_hits (include/aligntools_hip.h; kernels in at_scanhits.hip;
 * the sweep that produces the candidates is at_scan<W, true>, at_scan.hip.h; the rule is at_scanhits.h).  Per slice of pairs:
 *   sort                 the n candidate records by key = (pair << 32) | last column of the run (rocprim's radix sort over the bits in use).  The keys
 *                        are unique, so the order -- and everything behind it -- does not depend on the order the appends landed in
 *   at_scanhits_mark_k   flag[i] = candidate i is an occurrence (valley) that the separation of its query keeps
 *   (at_scan_tiles / at_scan_nops of at_render.hip.h: the exclusive prefix sums of the flags)
 *   at_scanhits_emit_k   the kept candidates, in key order, as ScanHit records (query, target, strand, distance, column) at their
 *                        prefix sums, and the per-query counts
 */
#pragma once
#include <hip/hip_runtime.h>
#include "at_scanhits.h"

namespace at {

struct ScanHitsArgs {
	long long n;                   /* sorted candidates of the slice */
	const unsigned long long *key;
	const int *val;
	long long s0, ntb;             /* the slice's first pair of its block; pair x = (entry qa + x / ntb, target x % ntb), as ScanArgs */
	int qa, enc, nrev0, min_sep;
	const int *qperm;
	const int *slen;
	int *flag;                     /* [n] 0 / 1 */
	const long long *off;          /* [n + 1] prefix sums of flag */
	ScanHit *hits;                 /* [off[n]] */
	int *qcount;                   /* [nq] += the kept hits of each query */
};

}   // namespace at

/* at_scanhits.hip (asynchronous on s; they return the launch's error).  at_scanhits_sort with tmp == NULL only sets *tmp_bytes */
extern "C" hipError_t at_scanhits_sort(void *tmp, size_t *tmp_bytes, const unsigned long long *key_in, unsigned long long *key_out,
                                       const int *val_in, int *val_out, long long n, long long npairs, hipStream_t s);
extern "C" hipError_t at_scanhits_mark_launch(const at::ScanHitsArgs *a, int ncu, hipStream_t s);
extern "C" hipError_t at_scanhits_emit_launch(const at::ScanHitsArgs *a, int ncu, hipStream_t s);
