/* at_search.hip -- the search's descriptor and merge kernels and their launches (at_search.hip.h) */
#include "at_search.hip.h"

#include <algorithm>

namespace at {

__global__ __launch_bounds__(256) void at_search_desc_k(const SearchDescArgs a)
{
	const long long stride = (long long)gridDim.x * blockDim.x;
	for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < a.n; p += stride) {
		const long long x = a.s0 + p;
		const long long qi = x / a.ntb, ti = x - qi * a.ntb;
		const int e = a.qperm[a.qa + qi], t = a.nq + a.tperm[a.ta + ti];
		const int q = a.enc ? ((e & 1) ? a.nrev0 + (e >> 1) : e >> 1) : e;
		a.woff1[p] = a.swoff[q]; a.len1[p] = a.slen[q];
		a.woff2[p] = a.swoff[t]; a.len2[p] = a.slen[t];
	}
}

/* one compare-exchange across lanes lane ^ j: the lane keeps the larger key when `hi`, else the smaller, with its payload */
__device__ __forceinline__ void search_cx(unsigned long long &key, int &ei, int &ej, int &st, int j, bool hi)
{
	const unsigned long long ok = __shfl_xor(key, j, 64);
	const int oei = __shfl_xor(ei, j, 64), oej = __shfl_xor(ej, j, 64), ost = __shfl_xor(st, j, 64);
	if (hi ? ok > key : ok < key) { key = ok; ei = oei; ej = oej; st = ost; }
}

/* Four wavefronts per workgroup, one caller query each.  The query's candidates in the slice are one contiguous run of pairs (with
 * both strands: the run of its two adjacent entries, so no other wavefront touches its list); they are taken 64 at a time (one per
 * lane).  A batch none of whose keys beats the list's K-th entry is skipped (one ballot: the common
 * case once the list has filled); otherwise the batch is sorted descending across the wave (bitonic, __shfl_xor), reversed against
 * the list (lane i: the larger of list[i] and batch[63 - i], a bitonic sequence holding the top 64 of both) and merged (bitonic). */
__global__ __launch_bounds__(256) void at_search_merge_k(const SearchMergeArgs a)
{
	const int lane = threadIdx.x & 63;
	const int w = (int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
	if (w >= a.nqs) return;                                   /* (wave-uniform) */
	const long long gs = a.ntb << a.two;                      /* pairs of one caller query in the block */
	const long long g = a.s0 / gs + w;                        /* the caller query's index in the block */
	const int q = a.qperm[a.qa + (g << a.two)] >> a.enc;
	const long long lo = g * gs > a.s0 ? g * gs : a.s0;
	const long long hi_ = (g + 1) * gs < a.s0 + a.n ? (g + 1) * gs : a.s0 + a.n;
	const size_t base = (size_t)q * a.k;
	unsigned long long key = 0;
	int ei = 0, ej = 0, st = 0;
	if (lane < a.k) { key = a.lkey[base + lane]; ei = a.lei[base + lane]; ej = a.lej[base + lane]; st = a.lst[base + lane]; }
	bool changed = false;
	int bad = 0;
	for (long long c0 = lo; c0 < hi_; c0 += 64) {
		const long long c = c0 + lane;
		unsigned long long ck = 0;
		int cei = 0, cej = 0, cst = 0;
		if (c < hi_) {
			const long long p = c - a.s0;
			const int s = a.score[p];
			if (s == INT32_MIN) bad = 1;
			else if (!a.use_cutoff || (a.is_edit ? s <= a.cutoff : s >= a.cutoff)) {
				const unsigned r = (unsigned)(a.is_edit ? -s : s) ^ 0x80000000u;   /* larger = better */
				const long long qi = (g << a.two) + (c - g * gs >= a.ntb);         /* the entry (query, strand) of the block */
				unsigned t = (unsigned)a.tperm[a.ta + (c - qi * a.ntb)];
				if (a.enc) t = (t << 1) | ((unsigned)a.qperm[a.qa + qi] & 1u);
				ck = ((unsigned long long)r << 32) | (unsigned long long)(~t);
				cei = a.end_i[p]; cej = a.end_j[p]; cst = a.state[p];
			}
		}
		const unsigned long long kth = __shfl(key, a.k - 1, 64);
		if (__ballot(ck > kth) == 0ull) continue;              /* nothing in this batch enters the list */
		/* bitonic sort of the batch, descending in lane order */
		for (int kk = 2; kk <= 64; kk <<= 1)
			for (int j = kk >> 1; j > 0; j >>= 1)
				search_cx(ck, cei, cej, cst, j, ((lane & j) == 0) == ((lane & kk) == 0));
		/* lane i: the larger of list[i] and batch[63 - i] -- the top 64 of the union, as a bitonic sequence */
		{
			const unsigned long long rk = __shfl(ck, 63 - lane, 64);
			const int rei = __shfl(cei, 63 - lane, 64), rej = __shfl(cej, 63 - lane, 64), rst = __shfl(cst, 63 - lane, 64);
			if (rk > key) { key = rk; ei = rei; ej = rej; st = rst; }
		}
		for (int j = 32; j > 0; j >>= 1) search_cx(key, ei, ej, st, j, (lane & j) == 0);
		if (lane >= a.k) { key = 0; ei = ej = st = 0; }        /* the list holds K entries, as in memory */
		changed = true;
	}
	if (__ballot(bad) != 0ull && lane == 0) *a.bad = 1;
	if (changed && lane < a.k) { a.lkey[base + lane] = key; a.lei[base + lane] = ei; a.lej[base + lane] = ej; a.lst[base + lane] = st; }
}

}   // namespace at

extern "C" hipError_t at_search_desc_launch(const at::SearchDescArgs *a, int ncu, hipStream_t s)
{
	const unsigned grid = (unsigned)std::max<long long>(1, std::min<long long>((a->n + 255) / 256, 8LL * ncu));
	hipLaunchKernelGGL(at::at_search_desc_k, dim3(grid), dim3(256), 0, s, *a);
	return hipGetLastError();
}

extern "C" hipError_t at_search_merge_launch(const at::SearchMergeArgs *a, hipStream_t s)
{
	const unsigned grid = (unsigned)((a->nqs + 3) / 4);
	hipLaunchKernelGGL(at::at_search_merge_k, dim3(grid), dim3(256), 0, s, *a);
	return hipGetLastError();
}
