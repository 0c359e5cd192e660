#include "at_edit_tb.hip.h"
#include "../../../include/aligntools_hip.h"
/* edit alignments on the bit-parallel path: the rule, the slab and the walk are described in at_edit_tb.hip.h */
namespace at {

template <int W>
__global__ __launch_bounds__(64) void at_edit_tb(const EditTbArgs ea)
{
	const MyersArgs &a = ea.m;
	const int lane = threadIdx.x;
	const int nw2max = (((a.max_l2 + 15) >> 4) + 2) | 1;   /* odd: the windows of the 64 lanes start in different LDS banks */
	uint32_t *ref = at_lds + lane * nw2max;                /* my alignment's s2 words */
	uint32_t *slab = ea.slab + (size_t)blockIdx.x * (size_t)ea.slab_words + lane;   /* [column - 1][word][plane][lane] */
	const long long nwork = (a.npairs + 63) / 64;
	long long wnext = blockIdx.x;
	while (wnext < nwork) {
		const long long wk = wnext;
		wnext = next_work(a.queue, lane);
		const long long pin = wk * 64 + lane;
		const bool have = pin < a.npairs;
		const long long p = a.order ? (long long)a.order[have ? pin : a.npairs - 1] : (have ? pin : a.npairs - 1);
		const int l1 = a.len1[p], l2 = a.len2[p];
		const uint32_t *q = a.seq + a.woff1[p], *r = a.seq + a.woff2[p];
		/* (a pair beyond the caller's bounds is refused: its ops slot and the slab are sized from them) */
		const bool fits = l1 >= 0 && l2 >= 0 && l1 <= 32 * W && l1 <= a.max_l1 && l2 <= a.max_l2;
		/* ---- stage s2 ---- */
		const int nw2 = fits ? (l2 + 15) >> 4 : 0;
		for (int w = 0; w < nw2; ++w) ref[w] = r[w];
		/* ---- my W words of s1 as two bit planes, all-ones vertical state (D(i,0) = i) ---- */
		uint32_t B0[W], B1[W], Pv[W], Mv[W];
		const int nw1 = fits ? (l1 + 15) >> 4 : 0;
#pragma unroll
		for (int w = 0; w < W; ++w) {
			const uint32_t lo = 2 * w < nw1 ? q[2 * w] : 0u, hi = 2 * w + 1 < nw1 ? q[2 * w + 1] : 0u;
			B0[w] = even16(lo) | (even16(hi) << 16);
			B1[w] = even16(lo >> 1) | (even16(hi >> 1) << 16);
			Pv[w] = 0xffffffffu; Mv[w] = 0u;
		}
		__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   /* LDS writes of this wave before its reads */
		const bool go = fits && have;
		/* ---- fill: the word step of at_myers<W, 1>; the lanes step together, the longest l2 decides the trip count ---- */
		const int steps_mine = (go && l1 > 0 && l2 > 0) ? l2 : 0;
		int nsteps = steps_mine;
#pragma unroll
		for (int d = 32; d >= 1; d >>= 1) nsteps = imax(nsteps, __shfl_xor(nsteps, d));
		uint32_t cw = 0;                                   /* the sixteen codes of s2 around column t */
		for (int t = 0; t < nsteps; ++t) {
			if ((t & 15) == 0) cw = t < l2 ? ref[t >> 4] : 0u;
			const uint32_t c = cw;
			cw >>= 2;
			if (t < steps_mine) {
				uint32_t pP = 0x80000000u, pM = 0u;        /* the border row: D(0,j) - D(0,j-1) = +1 */
				const uint32_t nC0 = (c & 1u) - 1u, nC1 = ((c >> 1) & 1u) - 1u;   /* ~(bit of the code spread over the word) */
				uint32_t *col = slab + (size_t)t * (W * 128);   /* column t + 1 */
#pragma unroll
				for (int w = 0; w < W; ++w) {
					const uint32_t Eq = (B0[w] ^ nC0) & (B1[w] ^ nC1);
					const uint32_t Eqh = Eq | (pM >> 31);      /* hin < 0 */
					const uint32_t sum = (Eqh & Pv[w]) + Pv[w];
					const uint32_t Xh = (sum ^ Pv[w]) | Eqh;
					const uint32_t Ph = Mv[w] | ~(Xh | Pv[w]);
					const uint32_t Mh = Pv[w] & Xh;
					const uint32_t Phs = __builtin_amdgcn_alignbit(Ph, pP, 31);   /* (Ph << 1) | hin > 0 */
					const uint32_t Mhs = __builtin_amdgcn_alignbit(Mh, pM, 31);
					const uint32_t Xv = Eq | Mv[w];
					Pv[w] = Mhs | ~(Xv | Phs);
					Mv[w] = Phs & Xv;
					pP = Ph; pM = Mh;
					col[(2 * w) * 64] = Pv[w];
					col[(2 * w + 1) * 64] = Mv[w];
				}
			}
		}
		/* ---- D(l1, l2) = l2 + the vertical differences of the last column over rows 1 .. l1 ---- */
		int sum = 0;
#pragma unroll
		for (int w = 0; w < W; ++w) {
			const int valid = l1 - 32 * w;                 /* rows of this word inside s1 */
			const uint32_t vm = valid >= 32 ? 0xffffffffu : valid <= 0 ? 0u : ((1u << valid) - 1u);
			sum += __popc(Pv[w] & vm) - __popc(Mv[w] & vm);
		}
		const int d = (l1 <= 0 || l2 <= 0) ? imax(l1, 0) + imax(l2, 0) : l2 + sum;
		if (have) {
			a.score[p] = fits ? d : INT32_MIN;
			if (a.end_i) a.end_i[p] = l1;
			if (a.end_j) a.end_j[p] = l2;
			if (a.state) a.state[p] = AT_ST_MID;
			if (!fits) a.nops[p] = -1;
		}
		/* ---- walk: a lane reads back the words it stored itself ---- */
		asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
		auto ldw = [&](int c, int w, uint32_t &P, uint32_t &M) {      /* column c >= 1 */
			const uint32_t *x = slab + ((size_t)(c - 1) * W + w) * 128;
			P = __hip_atomic_load(x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			M = __hip_atomic_load(x + 64, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		};
		auto ldcol = [&](int c, int w, uint32_t &P, uint32_t &M) {
			if (c >= 1) ldw(c, w, P, M);
			else { P = 0xffffffffu; M = 0u; }                         /* column 0 */
		};
		/* D(i, c) for c >= 0; leaves the word of row i of column c in P / M (i > 0) */
		auto dcol = [&](int i, int c, uint32_t &P, uint32_t &M) -> int {
			if (c <= 0) { P = 0xffffffffu; M = 0u; return i; }
			int s = c;
			const int wi = (i - 1) >> 5;                              /* i = 0: no word */
			for (int w = 0; w <= wi; ++w) {
				ldw(c, w, P, M);
				const int valid = i - 32 * w;
				const uint32_t vm = valid >= 32 ? 0xffffffffu : ((1u << valid) - 1u);
				s += __popc(P & vm) - __popc(M & vm);
			}
			return s;
		};
		int i = l1, j = l2, k = 0, A = d, B = 0;
		uint32_t cP = 0xffffffffu, cM = 0u, pP = 0xffffffffu, pM = 0u;   /* row i's word of the columns j and j - 1 */
		uint8_t *op = ea.ops + ea.ops_off[p];
		const int kmax = go ? l1 + l2 : 0;
		if (go) {
			if (i > 0) ldcol(j, (i - 1) >> 5, cP, cM);
			B = dcol(i, j - 1, pP, pM);
		}
		while (__any(go && (i > 0 || j > 0) && k < kmax)) {
			if (go && (i > 0 || j > 0) && k < kmax) {
				const int bi = (i - 1) & 31, wi = (i - 1) >> 5;
				const int dvc = i > 0 ? (int)((cP >> bi) & 1u) - (int)((cM >> bi) & 1u) : 0;
				const int dvp = i > 0 ? (int)((pP >> bi) & 1u) - (int)((pM >> bi) & 1u) : 0;
				bool mid = false;
				if (i > 0 && j > 0) {
					const uint32_t c1 = (q[(i - 1) >> 4] >> (((i - 1) & 15) * 2)) & 3u;
					const uint32_t c2 = (ref[(j - 1) >> 4] >> (((j - 1) & 15) * 2)) & 3u;
					mid = B - dvp + (c1 != c2 ? 1 : 0) == A;
				}
				const int code = mid ? AT_OP_MID : (i > 0 && dvc == 1) ? AT_OP_LOW : AT_OP_UPP;
				op[k++] = (uint8_t)code;
				if (code == AT_OP_LOW) {
					A -= dvc; B -= dvp; --i;
					const int wn = (i - 1) >> 5;
					if (i > 0 && wn != wi) { ldcol(j, wn, cP, cM); ldcol(j - 1, wn, pP, pM); }
				} else {
					A = mid ? B - dvp : B;
					if (mid) --i;
					--j;
					const int wn = (i - 1) >> 5;
					if (i > 0) {
						if (wn == wi) { cP = pP; cM = pM; }
						else ldcol(j, wn, cP, cM);
					}
					B = dcol(i, j - 1, pP, pM);
				}
			}
		}
		if (go) a.nops[p] = k;
		__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   /* the LDS region is reused by the next item */
	}
}

} /* namespace at */

at_edit_tb_fn at_pick_edit_tb(int w)
{
	return w == 2 ? at::at_edit_tb<2> : w == 3 ? at::at_edit_tb<3> : w == 4 ? at::at_edit_tb<4> : w == 5 ? at::at_edit_tb<5> : w == 8 ? at::at_edit_tb<8>
	     : w == 16 ? at::at_edit_tb<16> : w == 32 ? at::at_edit_tb<32> : nullptr;
}
