/* at_pairhits.hip -- the selection, descriptor and check kernels of at_allpairs_hits and their launches (at_pairhits.hip.h has the stages) */
#include "at_pairhits.hip.h"
#include "at_sweep.hip.h"

#include <algorithm>
#include <climits>

namespace at {

__global__ __launch_bounds__(256) void at_pairhits_flag_k(const PairHitsArgs a)
{
	const long long stride = (long long)gridDim.x * blockDim.x;
	unsigned long long bad = kPairHitsNoBad;
	for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < a.n; p += stride) {
		const int sc = a.score[p], st = a.state[p];
		if (sc == INT_MIN && (unsigned long long)(a.first + p) < bad) bad = (unsigned long long)(a.first + p);
		const bool over = a.is_edit ? sc <= a.threshold : sc >= a.threshold;
		a.flag[p] = (st != 0 && sc != INT_MIN && over) ? 1 : 0;
	}
	if (bad != kPairHitsNoBad) atomicMin(a.slots, bad);
}

__global__ __launch_bounds__(256) void at_pairhits_emit_k(const PairHitsArgs a)
{
	const long long stride = (long long)gridDim.x * blockDim.x;
	const long long t0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
	if (t0 == 0) a.slots[1] = (unsigned long long)a.off[a.n];
	for (long long p = t0; p < a.n; p += stride) {
		if (!a.flag[p]) continue;
		const long long at = a.off[p];
		if (at < 0 || at >= a.cap) continue;               /* (off[p] < off[n] <= n <= cap: never taken) */
		long long ia, ib;
		tri_pair(a.first + p, a.nreads, ia, ib);
		PairHit hit;
		hit.pair = a.first + p; hit.a = (int)ia; hit.b = (int)ib;
		hit.score = a.score[p]; hit.end_i = a.end_i[p]; hit.end_j = a.end_j[p]; hit.state = a.state[p];
		a.hits[at] = hit;
	}
}

__global__ __launch_bounds__(256) void at_pairhits_desc_k(const PairHitsDescArgs a)
{
	const long long stride = (long long)gridDim.x * blockDim.x;
	for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += stride) {
		const int ra = a.hits[i].a, rb = a.hits[i].b;
		const int l1 = a.slen[ra], l2 = a.slen[rb];
		a.woff1[i] = a.swoff[ra]; a.len1[i] = l1;
		a.woff2[i] = a.swoff[rb]; a.len2[i] = l2;
		a.nslot[i] = l1 + l2;
	}
}

__global__ __launch_bounds__(256) void at_pairhits_check_k(const PairHitsDescArgs a)
{
	const long long stride = (long long)gridDim.x * blockDim.x;
	int bad = 0;
	for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += stride) {
		const PairHit x = a.hits[i];
		if (a.score2[i] != x.score || a.end_i2[i] != x.end_i || a.end_j2[i] != x.end_j) bad = 1;
	}
	if (bad) atomicOr(a.bad, 1);
}

}   // namespace at

static unsigned pairhits_grid(long long n, int ncu) { return (unsigned)std::max<long long>(1, std::min<long long>((n + 255) / 256, 8LL * ncu)); }

extern "C" hipError_t at_pairhits_flag_launch(const at::PairHitsArgs *a, int ncu, hipStream_t s)
{
	hipLaunchKernelGGL(at::at_pairhits_flag_k, dim3(pairhits_grid(a->n, ncu)), dim3(256), 0, s, *a);
	return hipGetLastError();
}

extern "C" hipError_t at_pairhits_emit_launch(const at::PairHitsArgs *a, int ncu, hipStream_t s)
{
	hipLaunchKernelGGL(at::at_pairhits_emit_k, dim3(pairhits_grid(a->n, ncu)), dim3(256), 0, s, *a);
	return hipGetLastError();
}

extern "C" hipError_t at_pairhits_desc_launch(const at::PairHitsDescArgs *a, int ncu, hipStream_t s)
{
	hipLaunchKernelGGL(at::at_pairhits_desc_k, dim3(pairhits_grid(a->n, ncu)), dim3(256), 0, s, *a);
	return hipGetLastError();
}

extern "C" hipError_t at_pairhits_check_launch(const at::PairHitsDescArgs *a, int ncu, hipStream_t s)
{
	hipLaunchKernelGGL(at::at_pairhits_check_k, dim3(pairhits_grid(a->n, ncu)), dim3(256), 0, s, *a);
	return hipGetLastError();
}
