/* at_tilescan.hip -- the kernels around the sweep of a local scan and of a fit scan and their launches (at_tilescan.hip.h) */
#include "at_tilescan.hip.h"

#include <algorithm>
#include <climits>

namespace at {

/* the read entry e of qperm -> its read of the read set */
__device__ __forceinline__ int tilescan_query_read(int e, int enc, int nrev0) { return enc ? ((e & 1) ? nrev0 + (e >> 1) : e >> 1) : e; }

template <bool FIT>
__global__ __launch_bounds__(256) void at_tilescan_desc_k(const TileScanArgs a)
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
		const int qr = tilescan_query_read(a.qperm[a.qa + qi], a.enc, a.nrev0), tr = a.nq + (FIT ? a.tperm[a.ta + ti] : (int)ti);
		const int l2 = a.slen[tr], l1 = FIT ? a.slen[qr] : 0;   /* (local needs the query's length for a swept tile only) */
		/* the swept tile of the pass -> its tile (the repeats of tile 0 are not swept: at_localscan_plan.h; a block of a fit scan has
		 * no target shorter than its queries, so fit's cut is the local one) */
		const long long k = rest - a.tpre[lo] + (a.ragged ? localscan_swept_full(l2, a.tile, a.overlap) : 0);
		const long long n = localscan_swept_tile(k, localscan_dropped(l2, a.tile, a.overlap));
		const long long s0 = localscan_tile_start(n, a.tile, a.overlap), e = localscan_tile_end(n, a.tile, a.overlap, l2);
		const bool ok = p >= 0 && p < a.npairs && (FIT ? e - s0 >= l1 && l1 >= 1 : e > s0);   /* (the host's item range rules the rest out) */
		a.woff1[x] = a.swoff[qr]; a.len1[x] = !ok ? 0 : FIT ? l1 : a.slen[qr];
		a.woff2[x] = a.swoff[tr] + (ok ? s0 / a.bpw : 0); a.len2[x] = ok ? (int)(e - s0) : 0;
		a.s0[x] = s0; a.slot[x] = ok ? p : -1;
	}
}

__global__ __launch_bounds__(256) void at_tilescan_init_k(const TileScanArgs a)
{
	const long long stride = (long long)gridDim.x * blockDim.x;
	for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < a.npairs && p < a.cap; p += stride) a.key[p] = ~0ull;
}

template <bool FIT>
__global__ __launch_bounds__(256) void at_tilescan_fold_k(const TileScanArgs a)
{
	const long long stride = (long long)gridDim.x * blockDim.x;
	for (long long x = (long long)blockIdx.x * blockDim.x + threadIdx.x; x < a.nitems && x < a.cap; x += stride) {
		const long long p = a.slot[x];
		if (p < 0 || p >= a.npairs) { *a.bad = 1; continue; }
		if constexpr (FIT) {
			const int sc = a.score[x], ej = a.end_j[x], st = a.state[x];
			const long long aj = a.s0[x] + ej;
			if (sc == INT_MIN || ej < 0 || (st != AT_ST_MID && st != AT_ST_LOW) || !fitscan_key_ok(sc, aj)) { *a.bad = 1; continue; }
			atomicMin(a.key + p, fitscan_key(sc, st == AT_ST_LOW, aj));
		} else {
			const int sc = a.score[x], ei = a.end_i[x], ej = a.end_j[x];
			const long long aj = a.s0[x] + ej;
			if (sc == INT_MIN || sc < 0 || sc > kLocalScanSMax || ei < 0 || ei > kLocalScanMaxQuery || ej < 0 || aj > INT_MAX) { *a.bad = 1; continue; }
			atomicMin(a.key + p, localscan_key(sc, ei, aj));
		}
	}
}

template <bool FIT>
__global__ __launch_bounds__(256) void at_tilescan_unpack_k(const TileScanArgs a)
{
	const long long stride = (long long)gridDim.x * blockDim.x;
	for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < a.npairs && p < a.cap; p += stride) {
		const unsigned long long key = a.key[p];
		const bool none = key == ~0ull;                /* no tile folded: the merge raises the flag */
		if constexpr (FIT) {
			const int qr = tilescan_query_read(a.qperm[a.qa + (a.p0 + p) / a.ntb], a.enc, a.nrev0);
			a.o_score[p] = none ? INT_MIN : fitscan_key_score(key);
			a.o_end_i[p] = none ? 0 : a.slen[qr];          /* fit ends in the query's last row */
			a.o_end_j[p] = none ? 0 : fitscan_key_end_j(key);
			a.o_state[p] = none || !fitscan_key_low(key) ? AT_ST_MID : AT_ST_LOW;
		} else {
			a.o_score[p] = none ? INT_MIN : localscan_key_score(key);
			a.o_end_i[p] = none ? 0 : localscan_key_end_i(key);
			a.o_end_j[p] = none ? 0 : localscan_key_end_j(key);
			a.o_state[p] = AT_ST_MID;
		}
	}
}

/* a list entry's hit: (score, strand, target) of its key (at_search.hip.h); false for an empty entry */
__device__ __forceinline__ bool tilescan_hit(unsigned long long key, int enc, int &score, int &strand, int &target)
{
	if (!key) return false;
	score = (int)((unsigned)(key >> 32) ^ 0x80000000u);
	const unsigned low = ~(unsigned)key;
	target = (int)(low >> enc);
	strand = enc ? (int)(low & 1u) : 0;
	return true;
}

template <bool FIT>
__global__ __launch_bounds__(256) void at_tilescan_window_k(const TileScanWindowArgs a)
{
	const long long stride = (long long)gridDim.x * blockDim.x;
	for (long long x = (long long)blockIdx.x * blockDim.x + threadIdx.x; x < a.n; x += stride) {
		const long long e = a.eidx[x];
		int score = 0, strand = 0, target = 0;
		bool ok = e >= 0 && e < a.nlist && tilescan_hit(a.lkey[e], a.enc, score, strand, target);
		int qr = 0, l1 = 1, l2 = 1, ej = 0;
		if (ok) {
			qr = strand ? a.nrev0 + (int)(e / a.k) : (int)(e / a.k);
			l1 = a.slen[qr]; ej = a.lej[e];
			if constexpr (FIT) {
				l2 = a.slen[a.nq + target];
				ok = l1 >= 1 && l1 <= l2 && ej >= 0 && ej < l2;
			}
		}
		if (!ok) {
			/* (the host lists used entries only) a pair of one base each, so that nothing behind this kernel meets an empty sequence */
			*a.bad = 1;
			a.woff1[x] = a.swoff[0]; a.woff2[x] = a.swoff[a.nq]; a.len1[x] = 1; a.len2[x] = 1; a.ws[x] = 0;
			continue;
		}
		/* the window (ws, we]: local's ends in the hit's column */
		const long long ws = FIT ? fitscan_window_start(ej, l1, score, a.m, a.u, a.o, a.e) : localscan_window_start(ej, a.lei[e], score, a.m, a.u, a.o, a.e);
		const long long we = FIT ? fitscan_window_end(ej, ws, l1, l2) : ej;
		a.woff1[x] = a.swoff[qr]; a.len1[x] = l1;
		a.woff2[x] = a.swoff[a.nq + target] + ws / a.bpw; a.len2[x] = (int)(we - ws);
		a.ws[x] = (int)ws;
	}
}

template <bool FIT>
__global__ __launch_bounds__(256) void at_tilescan_check_k(const TileScanWindowArgs a)
{
	const long long stride = (long long)gridDim.x * blockDim.x;
	for (long long x = (long long)blockIdx.x * blockDim.x + threadIdx.x; x < a.n; x += stride) {
		const long long e = a.eidx[x];
		int score = 0, strand = 0, target = 0;
		if (e < 0 || e >= a.nlist || !tilescan_hit(a.lkey[e], a.enc, score, strand, target)) { *a.bad = 1; continue; }
		const bool same = FIT ? a.w_state[x] == a.lst[e] : a.w_end_i[x] == a.lei[e];
		if (a.w_score[x] != score || !same || a.w_end_j[x] != a.lej[e] - a.ws[x] || a.ncigar[x] < 0) *a.bad = 1;
		else a.stats[x * 8 + AT_CG_START_J] += a.ws[x];
	}
}

}   // namespace at

static unsigned tilescan_grid(long long n, int ncu) { return (unsigned)std::max<long long>(1, std::min<long long>((n + 255) / 256, 8LL * ncu)); }

/* the family's kernel over n items */
template <typename Args>
static hipError_t tilescan_launch(int mode, void (*local)(const Args), void (*fit)(const Args), long long n, const Args *a, int ncu, hipStream_t s)
{
	if (mode != AT_MODE_LOCAL && mode != AT_MODE_FIT) return hipErrorInvalidValue;
	hipLaunchKernelGGL(mode == AT_MODE_FIT ? fit : local, dim3(tilescan_grid(n, ncu)), dim3(256), 0, s, *a);
	return hipGetLastError();
}

extern "C" hipError_t at_tilescan_desc_launch(int mode, const at::TileScanArgs *a, int ncu, hipStream_t s)
{
	if (a->nitems > a->cap || a->ntb < 1 || a->tall < 1 || (a->bpw != 16 && a->bpw != 4)) return hipErrorInvalidValue;
	return tilescan_launch(mode, at::at_tilescan_desc_k<false>, at::at_tilescan_desc_k<true>, a->nitems, a, ncu, s);
}

extern "C" hipError_t at_tilescan_init_launch(const at::TileScanArgs *a, int ncu, hipStream_t s)
{
	if (a->npairs > a->cap) return hipErrorInvalidValue;
	hipLaunchKernelGGL(at::at_tilescan_init_k, dim3(tilescan_grid(a->npairs, ncu)), dim3(256), 0, s, *a);
	return hipGetLastError();
}

extern "C" hipError_t at_tilescan_fold_launch(int mode, const at::TileScanArgs *a, int ncu, hipStream_t s)
{
	if (a->nitems > a->cap) return hipErrorInvalidValue;
	return tilescan_launch(mode, at::at_tilescan_fold_k<false>, at::at_tilescan_fold_k<true>, a->nitems, a, ncu, s);
}

extern "C" hipError_t at_tilescan_unpack_launch(int mode, const at::TileScanArgs *a, int ncu, hipStream_t s)
{
	if (a->npairs > a->cap || (mode == AT_MODE_FIT && a->ntb < 1)) return hipErrorInvalidValue;
	return tilescan_launch(mode, at::at_tilescan_unpack_k<false>, at::at_tilescan_unpack_k<true>, a->npairs, a, ncu, s);
}

extern "C" hipError_t at_tilescan_window_launch(int mode, const at::TileScanWindowArgs *a, int ncu, hipStream_t s)
{
	if (a->k < 1 || !a->eidx || a->n > a->nlist || (a->bpw != 16 && a->bpw != 4)) return hipErrorInvalidValue;
	return tilescan_launch(mode, at::at_tilescan_window_k<false>, at::at_tilescan_window_k<true>, a->n, a, ncu, s);
}

extern "C" hipError_t at_tilescan_check_launch(int mode, const at::TileScanWindowArgs *a, int ncu, hipStream_t s)
{
	if (!a->eidx || a->n > a->nlist) return hipErrorInvalidValue;
	return tilescan_launch(mode, at::at_tilescan_check_k<false>, at::at_tilescan_check_k<true>, a->n, a, ncu, s);
}
