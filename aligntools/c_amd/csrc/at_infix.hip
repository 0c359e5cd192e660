#include "at_infix.hip.h"
#include "../../../include/aligntools_hip.h"
/* edit infix mode on the bit-parallel path: the rule, the bottom-aligned rows, the slab and the walk are described in at_infix.hip.h */
namespace at {

/* bits of word w (rows 32 w + 1 .. 32 w + 32) among the first `pad` rows */
AT_DEV uint32_t infix_pad_word(int pad, int w)
{
	const int nb = pad - 32 * w;
	return nb >= 32 ? 0xffffffffu : nb <= 0 ? 0u : ((1u << nb) - 1u);
}

/* a | b | c in one instruction, spelled out: written plainly, hipcc shares Eq | pad between the two places that use it and pays a
 * sixteenth instruction per word step for it */
AT_DEV uint32_t infix_or3(uint32_t a, uint32_t b, uint32_t c)
{
	uint32_t r;
	asm("v_or3_b32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
	return r;
}

template <int W, bool TB>
__global__ __launch_bounds__(64) void at_infix(const InfixArgs ea)
{
	const MyersArgs &a = ea.m;
	const int lane = threadIdx.x;
	const int nw2max = (((a.max_l2 + 15) >> 4) + 2) | 1;   /* odd: the windows of the 64 lanes start in different LDS banks */
	uint32_t *ref = at_lds + lane * nw2max;                /* my alignment's s2 words */
	uint32_t *slab = TB ? ea.slab + (size_t)blockIdx.x * (size_t)ea.slab_words + lane : nullptr;   /* [column - 1][word][plane][lane] */
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
		/* (a pair beyond the caller's bounds is refused: its ops slot, the slab and the LDS windows are sized from them) */
		const bool fits = l1 >= 0 && l2 >= 0 && l1 <= 32 * W && l1 <= a.max_l1 && l2 <= a.max_l2;
		/* ---- stage s2 ---- */
		const int nw2 = fits ? (l2 + 15) >> 4 : 0;
		for (int w = 0; w < nw2; ++w) ref[w] = r[w];
		/* ---- my W words of s1 as two bit planes, row l1 in the last bit of word W - 1 (the load of at_myers' SEMI form); the pad rows
		 * in front are wildcards whose vertical state starts at 0, the real rows start at +1 (D(i,0) = i) ---- */
		uint32_t B0[W], B1[W], Pv[W], Mv[W], pad[W];
		const int nw1 = fits ? (l1 + 15) >> 4 : 0;
		const int npad = 32 * W - (fits ? l1 : 0);
#pragma unroll
		for (int w = 0; w < W; ++w) {
			const int P = 32 * w - npad, kq = P >> 4, sh = (P & 15) * 2;
			const uint32_t x0 = kq >= 0 && kq < nw1 ? q[kq] : 0u, x1 = kq + 1 >= 0 && kq + 1 < nw1 ? q[kq + 1] : 0u;
			const uint32_t x2 = kq + 2 >= 0 && kq + 2 < nw1 ? q[kq + 2] : 0u;
			const uint32_t lo = __builtin_amdgcn_alignbit(x1, x0, sh), hi = __builtin_amdgcn_alignbit(x2, x1, sh);
			B0[w] = even16(lo) | (even16(hi) << 16);
			B1[w] = even16(lo >> 1) | (even16(hi >> 1) << 16);
			pad[w] = infix_pad_word(npad, w);
			Pv[w] = ~pad[w]; Mv[w] = 0u;
		}
		__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   /* LDS writes of this wave before its reads */
		const bool go = fits && have;
		/* ---- fill: the word step of at_myers<W, 1> with a zero top border; the lanes step together, the longest l2 decides the trip count ---- */
		const int steps_mine = (go && l1 > 0 && l2 > 0) ? l2 : 0;
		int nsteps = steps_mine;
#pragma unroll
		for (int d = 32; d >= 1; d >>= 1) nsteps = imax(nsteps, __shfl_xor(nsteps, d));
		uint32_t cw = 0;                                   /* the sixteen codes of s2 around column t */
		int d = fits ? l1 : 0, best = d, best_j = 0;       /* D(l1, column), its minimum so far and the first column that has it */
		for (int t = 0; t < nsteps; ++t) {
			if ((t & 15) == 0) cw = t < l2 ? ref[t >> 4] : 0u;
			const uint32_t c = cw;
			cw >>= 2;
			if (t < steps_mine) {                          /* inside my own l2 */
				uint32_t pP = 0u, pM = 0u;                     /* the border row: D(0,j) - D(0,j-1) = 0 */
				const uint32_t nC0 = (c & 1u) - 1u, nC1 = ((c >> 1) & 1u) - 1u;   /* ~(bit of the code spread over the word) */
				uint32_t *col = TB ? slab + (size_t)t * (W * 128) : nullptr;   /* column t + 1 */
#pragma unroll
				for (int w = 0; w < W; ++w) {
					const uint32_t Eq = (B0[w] ^ nC0) & (B1[w] ^ nC1);
					const uint32_t Eqh = infix_or3(Eq, pad[w], pM >> 31);   /* a wildcard row, or hin < 0 */
					const uint32_t sum = (Eqh & Pv[w]) + Pv[w];
					const uint32_t Xh = (sum ^ Pv[w]) | Eqh;
					const uint32_t Ph = Mv[w] | ~(Xh | Pv[w]);
					const uint32_t Mh = Pv[w] & Xh;
					const uint32_t Phs = __builtin_amdgcn_alignbit(Ph, pP, 31);   /* (Ph << 1) | hin > 0 */
					const uint32_t Mhs = __builtin_amdgcn_alignbit(Mh, pM, 31);
					const uint32_t Xv = infix_or3(Eq, pad[w], Mv[w]);
					Pv[w] = Mhs | ~(Xv | Phs);
					Mv[w] = Phs & Xv;
					pP = Ph; pM = Mh;
					/* (32 words, number only: left alone the scheduler interleaves the word steps until 256 VGPRs and 5 AGPRs are
					 * live, one wave per SIMD; kept to four word steps at a time it needs 217) */
					if constexpr (W == 32 && !TB) { if ((w & 3) == 3) __builtin_amdgcn_sched_barrier(0); }
					if constexpr (TB) {
						col[(2 * w) * 64] = Pv[w];
						col[(2 * w + 1) * 64] = Mv[w];
					}
				}
				/* the last word's horizontal difference in its last row = D(l1, t + 1) - D(l1, t) */
				d += (int)(pP >> 31) - (int)(pM >> 31);
				if (d < best) { best = d; best_j = t + 1; }
			}
		}
		if constexpr (TB) {
			/* end anchored (at_scan_hits' windows): the end cell is (l1, l2) with the value the fill ended on, whatever the minimum is */
			if (ea.anchor_end && fits) { best = d; best_j = l2; }
		}
		if (have) {
			if (fits) {
				a.score[p] = best;
				if (a.end_i) a.end_i[p] = l1;
				if (a.end_j) a.end_j[p] = best_j;
				if (a.state) a.state[p] = AT_ST_MID;
				if (!TB && a.nops) a.nops[p] = 0;
			} else {
				a.score[p] = INT32_MIN;
				if (a.nops) a.nops[p] = -1;
			}
		}
		if constexpr (TB) {
			/* ---- walk: a lane reads back the words it stored itself; rows in padded coordinates (ip = npad + i) ---- */
			asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
			const int w0 = npad >> 5;                                     /* the first word with a real row */
			auto ldw = [&](int c, int w, uint32_t &P, uint32_t &M) {      /* column c >= 1 */
				const uint32_t *x = slab + ((size_t)(c - 1) * W + w) * 128;
				P = __hip_atomic_load(x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
				M = __hip_atomic_load(x + 64, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			};
			auto ldcol = [&](int c, int w, uint32_t &P, uint32_t &M) {
				if (c >= 1) ldw(c, w, P, M);
				else { P = ~infix_pad_word(npad, w); M = 0u; }            /* column 0: +1 on every real row */
			};
			/* D(ip - npad, c) for c >= 0; leaves the word of row ip of column c in P / M (ip > npad) */
			auto dcol = [&](int ip, int c, uint32_t &P, uint32_t &M) -> int {
				const int wi = (ip - 1) >> 5;
				if (c <= 0) { if (ip > npad) { P = ~infix_pad_word(npad, wi); M = 0u; } return ip - npad; }
				int s = 0;                                                /* the top border: D(0, c) = 0 */
				for (int w = w0; w <= wi; ++w) {
					ldw(c, w, P, M);
					const int valid = ip - 32 * w;
					const uint32_t vm = valid >= 32 ? 0xffffffffu : ((1u << valid) - 1u);
					s += __popc(P & vm) - __popc(M & vm);
				}
				return s;
			};
			int ip = 32 * W, j = best_j, k = 0, A = best, B = 0;
			uint32_t cP = 0u, cM = 0u, pP = 0u, pM = 0u;                  /* row ip's word of the columns j and j - 1 */
			uint8_t *op = ea.ops + ea.ops_off[p];
			const int kmax = go ? l1 + l2 : 0;
			if (go && ip > npad) {
				ldcol(j, (ip - 1) >> 5, cP, cM);
				B = dcol(ip, j - 1, pP, pM);
			}
			while (__any(go && ip > npad && k < kmax)) {
				if (go && ip > npad && k < kmax) {
					const int bi = (ip - 1) & 31, wi = (ip - 1) >> 5;
					const int dvc = (int)((cP >> bi) & 1u) - (int)((cM >> bi) & 1u);
					const int dvp = (int)((pP >> bi) & 1u) - (int)((pM >> bi) & 1u);
					bool mid = false;
					if (j > 0) {
						const int i = ip - npad;
						const uint32_t c1 = (q[(i - 1) >> 4] >> (((i - 1) & 15) * 2)) & 3u;
						const uint32_t c2 = (ref[(j - 1) >> 4] >> (((j - 1) & 15) * 2)) & 3u;
						mid = B - dvp + (c1 != c2 ? 1 : 0) == A;
					}
					const int code = mid ? AT_OP_MID : dvc == 1 ? AT_OP_LOW : AT_OP_UPP;
					op[k++] = (uint8_t)code;
					if (code == AT_OP_LOW) {
						A -= dvc; B -= dvp; --ip;
						const int wn = (ip - 1) >> 5;
						if (ip > npad && wn != wi) { ldcol(j, wn, cP, cM); ldcol(j - 1, wn, pP, pM); }
					} else {
						A = mid ? B - dvp : B;
						if (mid) --ip;
						--j;
						const int wn = (ip - 1) >> 5;
						if (ip > npad) {
							if (wn == wi) { cP = pP; cM = pM; }
							else ldcol(j, wn, cP, cM);
						}
						B = dcol(ip, j - 1, pP, pM);
					}
				}
			}
			if (go) a.nops[p] = k;
		}
		__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   /* the LDS region is reused by the next item */
	}
}

} /* namespace at */

at_infix_fn at_pick_infix(int w, int tb)
{
	if (tb)
		return w == 2 ? at::at_infix<2, true> : w == 3 ? at::at_infix<3, true> : w == 4 ? at::at_infix<4, true> : w == 5 ? at::at_infix<5, true>
		     : w == 8 ? at::at_infix<8, true> : w == 16 ? at::at_infix<16, true> : w == 32 ? at::at_infix<32, true> : nullptr;
	return w == 2 ? at::at_infix<2, false> : w == 3 ? at::at_infix<3, false> : w == 4 ? at::at_infix<4, false> : w == 5 ? at::at_infix<5, false>
	     : w == 8 ? at::at_infix<8, false> : w == 16 ? at::at_infix<16, false> : w == 32 ? at::at_infix<32, false> : nullptr;
}
