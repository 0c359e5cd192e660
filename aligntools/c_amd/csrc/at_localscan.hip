/* at_localscan.hip -- the kernels around the sweep of a local scan and their launches (at_localscan.hip.h) */
#include "at_localscan.hip.h"

#include <algorithm>
#include <climits>

namespace at {

/* the read entry e of qperm -> its read of the read set */
__device__ __forceinline__ int localscan_query_read(int e, int enc, int nrev0) { return enc ? ((e & 1) ? nrev0 + (e >> 1) : e >> 1) : e; }

__global__ __launch_bounds__(256) void at_localscan_desc_k(const LocalScanArgs a)
{
	const long long stride = (long long)gridDim.x * blockDim.x;
	for (long long x = (long long)blockIdx.x * blockDim.x + threadIdx.x; x < a.nitems && x < a.cap; x += stride) {
		const long long y = a.y0 + x;
		const long long qi = y / a.tall, rest = y - qi * a.tall;
		long long lo = 0, hi = a.ntb;                  /* tpre[lo] <= rest < tpre[hi] */
		while (hi - lo > 1) {
			const long long mid = (lo + hi) >> 1;
			if (a.tpre[mid] <= rest) lo = mid; else hi = mid;
		}
		const long long ti = lo, p = qi * a.ntb + ti - a.p0;
		const int qr = localscan_query_read(a.qperm[a.qa + qi], a.enc, a.nrev0), tr = a.nq + (int)ti;
		const int l2 = a.slen[tr];
		/* the swept tile of the pass -> its tile (the repeats of tile 0 are not swept: at_localscan_plan.h) */
		const long long k = rest - a.tpre[lo] + (a.ragged ? localscan_swept_full(l2, a.tile, a.overlap) : 0);
		const long long n = localscan_swept_tile(k, localscan_dropped(l2, a.tile, a.overlap));
		const long long s0 = localscan_tile_start(n, a.tile, a.overlap), e = localscan_tile_end(n, a.tile, a.overlap, l2);
		const bool ok = p >= 0 && p < a.npairs && e > s0;   /* (the host's item range rules the rest out) */
		a.woff1[x] = a.swoff[qr]; a.len1[x] = ok ? a.slen[qr] : 0;
		a.woff2[x] = a.swoff[tr] + (ok ? s0 / a.bpw : 0); a.len2[x] = ok ? (int)(e - s0) : 0;
		a.s0[x] = s0; a.slot[x] = ok ? p : -1;
	}
}

__global__ __launch_bounds__(256) void at_localscan_init_k(const LocalScanArgs a)
{
	const long long stride = (long long)gridDim.x * blockDim.x;
	for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < a.npairs && p < a.cap; p += stride) a.key[p] = ~0ull;
}

__global__ __launch_bounds__(256) void at_localscan_fold_k(const LocalScanArgs a)
{
	const long long stride = (long long)gridDim.x * blockDim.x;
	for (long long x = (long long)blockIdx.x * blockDim.x + threadIdx.x; x < a.nitems && x < a.cap; x += stride) {
		const long long p = a.slot[x];
		if (p < 0 || p >= a.npairs) { *a.bad = 1; continue; }
		const int sc = a.score[x], ei = a.end_i[x], ej = a.end_j[x];
		const long long aj = a.s0[x] + ej;
		if (sc == INT_MIN || sc < 0 || sc > kLocalScanSMax || ei < 0 || ei > kLocalScanMaxQuery || ej < 0 || aj > INT_MAX) { *a.bad = 1; continue; }
		atomicMin(a.key + p, localscan_key(sc, ei, aj));
	}
}

__global__ __launch_bounds__(256) void at_localscan_unpack_k(const LocalScanArgs a)
{
	const long long stride = (long long)gridDim.x * blockDim.x;
	for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < a.npairs && p < a.cap; p += stride) {
		const unsigned long long key = a.key[p];
		const bool none = key == ~0ull;                /* no tile folded: the merge raises the flag */
		a.o_score[p] = none ? INT_MIN : localscan_key_score(key);
		a.o_end_i[p] = none ? 0 : localscan_key_end_i(key);
		a.o_end_j[p] = none ? 0 : localscan_key_end_j(key);
		a.o_state[p] = AT_ST_MID;
	}
}

/* a list entry's hit: (score, strand, target) of its key (at_search.hip.h); false for an empty entry */
__device__ __forceinline__ bool localscan_hit(unsigned long long key, int enc, int &score, int &strand, int &target)
{
	if (!key) return false;
	score = (int)((unsigned)(key >> 32) ^ 0x80000000u);
	const unsigned low = ~(unsigned)key;
	target = (int)(low >> enc);
	strand = enc ? (int)(low & 1u) : 0;
	return true;
}

__global__ __launch_bounds__(256) void at_localscan_window_k(const LocalScanWindowArgs a)
{
	const long long stride = (long long)gridDim.x * blockDim.x;
	for (long long x = (long long)blockIdx.x * blockDim.x + threadIdx.x; x < a.n; x += stride) {
		const long long e = a.eidx[x];
		int score = 0, strand = 0, target = 0;
		if (e < 0 || e >= a.nlist || !localscan_hit(a.lkey[e], a.enc, score, strand, target)) {
			/* (the host lists used entries only) a pair of one base each, so that nothing behind this kernel meets an empty sequence */
			*a.bad = 1;
			a.woff1[x] = a.swoff[0]; a.woff2[x] = a.swoff[a.nq]; a.len1[x] = 1; a.len2[x] = 1; a.ws[x] = 0;
			continue;
		}
		const int q = (int)(e / a.k), qr = strand ? a.nrev0 + q : q, ei = a.lei[e], ej = a.lej[e];
		const int ws = (int)localscan_window_start(ej, ei, score, a.m, a.u, a.o, a.e);
		a.woff1[x] = a.swoff[qr]; a.len1[x] = a.slen[qr];
		a.woff2[x] = a.swoff[a.nq + target] + ws / a.bpw; a.len2[x] = ej - ws;
		a.ws[x] = ws;
	}
}

__global__ __launch_bounds__(256) void at_localscan_check_k(const LocalScanWindowArgs a)
{
	const long long stride = (long long)gridDim.x * blockDim.x;
	for (long long x = (long long)blockIdx.x * blockDim.x + threadIdx.x; x < a.n; x += stride) {
		const long long e = a.eidx[x];
		int score = 0, strand = 0, target = 0;
		if (e < 0 || e >= a.nlist || !localscan_hit(a.lkey[e], a.enc, score, strand, target)) { *a.bad = 1; continue; }
		if (a.w_score[x] != score || a.w_end_i[x] != a.lei[e] || a.w_end_j[x] != a.lej[e] - a.ws[x] || a.ncigar[x] < 0) *a.bad = 1;
		else a.stats[x * 8 + AT_CG_START_J] += a.ws[x];
	}
}

}   // namespace at

static unsigned localscan_grid(long long n, int ncu) { return (unsigned)std::max<long long>(1, std::min<long long>((n + 255) / 256, 8LL * ncu)); }

extern "C" hipError_t at_localscan_desc_launch(const at::LocalScanArgs *a, int ncu, hipStream_t s)
{
	if (a->nitems > a->cap || a->ntb < 1 || a->tall < 1 || (a->bpw != 16 && a->bpw != 4)) return hipErrorInvalidValue;
	hipLaunchKernelGGL(at::at_localscan_desc_k, dim3(localscan_grid(a->nitems, ncu)), dim3(256), 0, s, *a);
	return hipGetLastError();
}

extern "C" hipError_t at_localscan_init_launch(const at::LocalScanArgs *a, int ncu, hipStream_t s)
{
	if (a->npairs > a->cap) return hipErrorInvalidValue;
	hipLaunchKernelGGL(at::at_localscan_init_k, dim3(localscan_grid(a->npairs, ncu)), dim3(256), 0, s, *a);
	return hipGetLastError();
}

extern "C" hipError_t at_localscan_fold_launch(const at::LocalScanArgs *a, int ncu, hipStream_t s)
{
	if (a->nitems > a->cap) return hipErrorInvalidValue;
	hipLaunchKernelGGL(at::at_localscan_fold_k, dim3(localscan_grid(a->nitems, ncu)), dim3(256), 0, s, *a);
	return hipGetLastError();
}

extern "C" hipError_t at_localscan_unpack_launch(const at::LocalScanArgs *a, int ncu, hipStream_t s)
{
	if (a->npairs > a->cap) return hipErrorInvalidValue;
	hipLaunchKernelGGL(at::at_localscan_unpack_k, dim3(localscan_grid(a->npairs, ncu)), dim3(256), 0, s, *a);
	return hipGetLastError();
}

extern "C" hipError_t at_localscan_window_launch(const at::LocalScanWindowArgs *a, int ncu, hipStream_t s)
{
	if (a->k < 1 || !a->eidx || a->n > a->nlist || (a->bpw != 16 && a->bpw != 4)) return hipErrorInvalidValue;
	hipLaunchKernelGGL(at::at_localscan_window_k, dim3(localscan_grid(a->n, ncu)), dim3(256), 0, s, *a);
	return hipGetLastError();
}

extern "C" hipError_t at_localscan_check_launch(const at::LocalScanWindowArgs *a, int ncu, hipStream_t s)
{
	if (!a->eidx || a->n > a->nlist) return hipErrorInvalidValue;
	hipLaunchKernelGGL(at::at_localscan_check_k, dim3(localscan_grid(a->n, ncu)), dim3(256), 0, s, *a);
	return hipGetLastError();
}
