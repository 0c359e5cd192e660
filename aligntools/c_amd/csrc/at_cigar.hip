/* at_cigar.hip -- the CIGAR kernel (count phase, write phase) and its launch (at_cigar.hip.h) */
#include "at_cigar.hip.h"
#include "at_seqbase.hip.h"

#include <algorithm>

namespace at {

constexpr int CG_NONE = 0xff;      /* the class of a lane without an op, and of "no run yet" */

template <int BITS, int W, int PHASE>
__global__ __launch_bounds__(256) void at_cigar_k(const CigarArgs a)
{
	constexpr int NGR = 64 / W;
	const int lane = threadIdx.x & 63, g = lane / W, lg = lane % W;
	const long long wave = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
	const long long nwaves = (long long)gridDim.x * (blockDim.x >> 6);
	const unsigned long long gm = W == 64 ? ~0ull : ((1ull << W) - 1ull) << (W * g);   /* my group's lanes */
	const unsigned long long lt = ((1ull << lg) - 1ull) << (W * g);                     /* ... below me */
	for (long long kk = wave * NGR; kk < a.npairs; kk += nwaves * NGR) {
		const long long k = kk + g;
		const bool valid = k < a.npairs;
		const int nraw = valid ? a.nops[k] : -1;               /* < 0: refused by the sweep kernel (or no pair) */
		int n = nraw < 0 ? 0 : nraw;
		int nc = 0;
		long long co = 0;
		if constexpr (PHASE == 1) {
			/* only pairs with runs that fit below the capacity are walked at all */
			nc = valid ? a.ncigar[k] : -1;
			if (nc > 0) co = a.cigar_off[k];
			if (nc <= 0 || co + nc > a.cap) n = 0;
		}
		int nmax = n;
#pragma unroll
		for (int d = W; d < 64; d <<= 1) nmax = max(nmax, __shfl_xor(nmax, d));
		long long oo = 0, w1 = 0, w2 = 0;
		int i = 0, j = 0;
		if (nraw >= 0) {
			oo = a.ops_off[k];
			w1 = a.woff1[k]; w2 = a.woff2[k];
			i = a.end_i[k]; j = a.end_j[k];
		}
		bool gbad = nraw >= 0 && (i < 0 || j < 0);             /* (uniform over the group) */
		int carry_cls = CG_NONE, carry_len = 0, runs = 0;
		int neq = 0, nx = 0, ni = 0, nd = 0, nn = 0, ngap = 0;
		for (int base = 0; base < nmax; base += W) {
			const int p = base + lg;
			const bool act = p < n && !gbad;
			const uint32_t op = act ? a.ops[oo + p] : 0xffu;
			const bool okop = act && op <= 3u;
			const bool di = okop && op <= 1u;                  /* MID, LOW consume a row    */
			const bool dj = okop && op != 1u;                  /* MID, UPP, JUMP a column   */
			const unsigned long long mi = __ballot(di), mj = __ballot(dj);
			const int ii = i - __popcll(mi & lt) - 1;
			const int jj = j - __popcll(mj & lt) - 1;
			const bool lanebad = act && (op > 3u || (di && ii < 0) || (dj && jj < 0));
			if (__ballot(lanebad) & gm) gbad = true;
			const bool live = act && !gbad;
			int cls = CG_NONE;                                 /* the column's class, '=' and 'X' apart */
			if (live) {
				if (op != 0u) cls = (int)op;
				else if (PHASE == 1 && a.merge) cls = 7;       /* (all the same to the runs: no base is read) */
				else cls = render_base<BITS>(a.seq, w1, ii) == render_base<BITS>(a.seq, w2, jj) ? 7 : 8;
			}
			const int rc = a.merge && live && cls >= 7 ? 0 : cls;   /* ... as the runs see it */
			int prev = __shfl_up(rc, 1, W);
			if (lg == 0) prev = carry_cls;
			const bool head = live && rc != prev;
			const unsigned long long hm = __ballot(head) & gm;
			const int nact = __popcll(__ballot(live) & gm);
			if constexpr (PHASE == 0) {
				neq += __popcll(__ballot(cls == 7) & gm);
				nx += __popcll(__ballot(cls == 8) & gm);
				ni += __popcll(__ballot(cls == 1) & gm);
				nd += __popcll(__ballot(cls == 2) & gm);
				nn += __popcll(__ballot(cls == 3) & gm);
				ngap += __popcll(__ballot(head && (cls == 1 || cls == 2)) & gm);
			} else {
				/* a head closes the run before it: that run began at the head below me in this pass, or was carried in */
				const unsigned long long below = hm & lt;
				const int r = runs + __popcll(below);          /* the number of the run I open = runs closed before me */
				if (head && r > 0 && r <= nc) {
					const int len = below ? lg - (63 - __clzll(below) - W * g) : carry_len + lg;
					a.cigar[co + nc - r] = ((uint32_t)len << 4) | (uint32_t)prev;
				}
			}
			runs += __popcll(hm);
			if (hm) carry_len = nact - (63 - __clzll(hm) - W * g);
			else carry_len += nact;
			const int lastcls = __shfl(rc, nact > 0 ? nact - 1 : 0, W);
			if (nact > 0) carry_cls = lastcls;
			i -= __popcll(mi & gm);
			j -= __popcll(mj & gm);
		}
		if constexpr (PHASE == 0) {
			const bool refused = nraw < 0 || gbad;
			if (valid && lg == 0) a.ncigar[k] = refused ? -1 : runs;
			if (valid && a.stats && lg < 8) {
				const int v = lg == 0 ? i : lg == 1 ? j : lg == 2 ? neq : lg == 3 ? nx : lg == 4 ? ni : lg == 5 ? nd : lg == 6 ? nn : ngap;
				a.stats[k * 8 + lg] = refused ? -1 : v;
			}
		} else {
			/* the run that reaches the START of the alignment: the first word */
			if (lg == 0 && n > 0 && !gbad && runs > 0 && runs <= nc) a.cigar[co + nc - runs] = ((uint32_t)carry_len << 4) | (uint32_t)carry_cls;
		}
	}
}

}   // namespace at

extern "C" hipError_t at_cigar_launch(const at::CigarArgs *a, int bits, int w, int phase, int ncu, hipStream_t s)
{
	if (a->npairs <= 0) return hipSuccess;
	const int per_block = 4 * (64 / w);
	const unsigned grid = (unsigned)std::max<long long>(1, std::min<long long>((a->npairs + per_block - 1) / per_block, 16LL * ncu));
#define AT_CIGAR(B, W, P) hipLaunchKernelGGL((at::at_cigar_k<B, W, P>), dim3(grid), dim3(256), 0, s, *a)
	if (bits == 2) {
		if (w == 64) { if (phase == 0) AT_CIGAR(2, 64, 0); else AT_CIGAR(2, 64, 1); }
		else { if (phase == 0) AT_CIGAR(2, 16, 0); else AT_CIGAR(2, 16, 1); }
	} else {
		if (w == 64) { if (phase == 0) AT_CIGAR(8, 64, 0); else AT_CIGAR(8, 64, 1); }
		else { if (phase == 0) AT_CIGAR(8, 16, 0); else AT_CIGAR(8, 16, 1); }
	}
#undef AT_CIGAR
	return hipGetLastError();
}
