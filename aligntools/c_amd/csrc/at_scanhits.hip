#include <cstring>
#include <rocprim/device/device_radix_sort.hpp>
#include "at_scanhits.hip.h"
/* the selection stage of at_scan_hits: at_scanhits.hip.h has the stages, at_scanhits.h the rule */
#include <algorithm>

namespace at {

/* the read entry of a sorted candidate's pair (qperm's encoding, at_scan.hip) */
static __device__ inline int scanhits_entry(const ScanHitsArgs &a, unsigned long long key)
{
	return a.qperm[a.qa + (a.s0 + scan_cand_pair(key)) / a.ntb];
}

__global__ __launch_bounds__(256) void at_scanhits_mark_k(const ScanHitsArgs a)
{
	const long long stride = (long long)gridDim.x * blockDim.x;
	for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += stride) {
		const int e = scanhits_entry(a, a.key[i]);
		const int qr = a.enc ? ((e & 1) ? a.nrev0 + (e >> 1) : e >> 1) : e;
		const long long sep = scan_hits_sep(a.min_sep, a.slen[qr]);
		a.flag[i] = scan_hit_kept((const uint64_t *)a.key, a.val, a.n, i, sep) ? 1 : 0;
	}
}

__global__ __launch_bounds__(256) void at_scanhits_emit_k(const ScanHitsArgs a)
{
	const long long stride = (long long)gridDim.x * blockDim.x;
	for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += stride) {
		if (!a.flag[i]) continue;
		const unsigned long long key = a.key[i];
		const int e = scanhits_entry(a, key);
		ScanHit hit;
		hit.query = a.enc ? e >> 1 : e;
		hit.strand = a.enc ? e & 1 : 0;
		hit.target = (int)((a.s0 + scan_cand_pair(key)) % a.ntb);
		hit.score = scan_cand_tail(a.val[i]);
		hit.end_j = (int)scan_cand_column(key);
		a.hits[a.off[i]] = hit;                        /* off[i] < off[n] <= n, the size of hits */
		atomicAdd(a.qcount + hit.query, 1);
	}
}

}   // namespace at

extern "C" hipError_t at_scanhits_sort(void *tmp, size_t *tmp_bytes, const unsigned long long *key_in, unsigned long long *key_out,
                                       const int *val_in, int *val_out, long long n, long long npairs, hipStream_t s)
{
	unsigned end_bit = 32;                                 /* the column, and the bits of the slice's pair indices */
	while (end_bit < 64 && (npairs - 1) >> (end_bit - 32)) ++end_bit;
	return rocprim::radix_sort_pairs(tmp, *tmp_bytes, key_in, key_out, val_in, val_out, (size_t)n, 0u, end_bit, s);
}

static unsigned scanhits_grid(long long n, int ncu) { return (unsigned)std::max<long long>(1, std::min<long long>((n + 255) / 256, 8LL * ncu)); }

extern "C" hipError_t at_scanhits_mark_launch(const at::ScanHitsArgs *a, int ncu, hipStream_t s)
{
	hipLaunchKernelGGL(at::at_scanhits_mark_k, dim3(scanhits_grid(a->n, ncu)), dim3(256), 0, s, *a);
	return hipGetLastError();
}

extern "C" hipError_t at_scanhits_emit_launch(const at::ScanHitsArgs *a, int ncu, hipStream_t s)
{
	hipLaunchKernelGGL(at::at_scanhits_emit_k, dim3(scanhits_grid(a->n, ncu)), dim3(256), 0, s, *a);
	return hipGetLastError();
}
