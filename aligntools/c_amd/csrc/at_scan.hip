#include "at_scan.hip.h"
#include "../../../include/aligntools_hip.h"
/* reads against long targets: the mapping, the tiles and the kernels around the sweep are described in at_scan.hip.h */
#include <algorithm>

namespace at {

AT_DEV uint32_t scan_pad_word(int pad, int w)
{
	const int nb = pad - 32 * w;
	return nb >= 32 ? 0xffffffffu : nb <= 0 ? 0u : ((1u << nb) - 1u);
}

/* a | b | c in one instruction (at_infix.hip has the reason); b is the wave-uniform pad word, in an SGPR or in a VGPR */
template <bool PAD_S>
AT_DEV uint32_t scan_or3(uint32_t a, uint32_t b, uint32_t c)
{
	uint32_t r;
	if constexpr (PAD_S) asm("v_or3_b32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "s"(b), "v"(c));
	else asm("v_or3_b32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
	return r;
}

/* the read entry e of qperm -> its read of the read set */
AT_DEV int scan_query_read(int e, int enc, int nrev0) { return enc ? ((e & 1) ? nrev0 + (e >> 1) : e >> 1) : e; }

/* HITS: no best / best_j and no slot; the descents of the last row in own columns at or under the cutoff (which the host sets to
 * c = min(max_dist, l1 - 1) per block) go to the slice's candidate buffer, one record per run of consecutive ones (at_scan.hip.h) */
template <int W, bool HITS>
__global__ __launch_bounds__(64) void at_scan(const ScanArgs a)
{
	constexpr bool PAD_S = W <= 16;                    /* 32 words: B0 / B1 take 64 SGPRs, the pad words stay in VGPRs */
	constexpr int kColsUnrolled = W <= 5 ? 4 : 1;      /* short reads: the loop's own instructions weigh against 14 W */
	const int lane = threadIdx.x;
	long long wnext = blockIdx.x;
	while (wnext < a.nitems) {
		const long long y = a.y0 + wnext;
		wnext = next_work(a.queue, lane);
		/* ---- the item: (query entry, target, group), all wave-uniform ---- */
		const long long qi = y / a.gall, rest = y - qi * a.gall;
		long long lo = 0, hi = a.ntb;                  /* gpre[lo] <= rest < gpre[hi] */
		while (hi - lo > 1) {
			const long long mid = (lo + hi) >> 1;
			if (a.gpre[mid] <= rest) lo = mid; else hi = mid;
		}
		const long long ti = lo, grp = rest - a.gpre[lo];
		const long long p = qi * a.ntb + ti - a.s0;
		if (p < 0 || p >= a.npairs) continue;          /* (not one of the slice's pairs: the host's item range rules it out) */
		const int qr = scan_query_read(a.qperm[a.qa + qi], a.enc, a.nrev0), tr = a.nq + (int)ti;
		const int l1 = uni(a.slen[qr]), l2 = uni(a.slen[tr]);
		if (l1 < 0 || l2 < 0 || l1 > 32 * W) continue; /* (refused by the host) */
		const uint32_t *q = a.seq + a.swoff[qr], *r = a.seq + a.swoff[tr];
		/* ---- the read's W words as two bit planes, row l1 in the last bit of word W - 1, wildcard pad rows in front (at_infix.hip) ---- */
		uint32_t B0[W], B1[W], pad[W], Pv[W], Mv[W];
		const int nw1 = (l1 + 15) >> 4, npad = 32 * W - l1;
#pragma unroll
		for (int w = 0; w < W; ++w) {
			const int P = 32 * w - npad, kq = P >> 4, sh = (P & 15) * 2;
			const uint32_t x0 = kq >= 0 && kq < nw1 ? q[kq] : 0u, x1 = kq + 1 >= 0 && kq + 1 < nw1 ? q[kq + 1] : 0u;
			const uint32_t x2 = kq + 2 >= 0 && kq + 2 < nw1 ? q[kq + 2] : 0u;
			const uint32_t xl = __builtin_amdgcn_alignbit(x1, x0, sh), xh = __builtin_amdgcn_alignbit(x2, x1, sh);
			B0[w] = (uint32_t)uni((int)(even16(xl) | (even16(xh) << 16)));
			B1[w] = (uint32_t)uni((int)(even16(xl >> 1) | (even16(xh >> 1) << 16)));
			pad[w] = PAD_S ? (uint32_t)uni((int)scan_pad_word(npad, w)) : scan_pad_word(npad, w);
			Pv[w] = ~pad[w]; Mv[w] = 0u;
		}
		/* ---- my tile: own columns (n T, (n + 1) T], swept from s0 ---- */
		const int ov = scan_overlap(l1, a.use_cutoff, a.cutoff);
		const long long n = grp * 64 + lane;
		const long long s0 = scan_tile_start(n, a.tile, ov), e = scan_tile_end(n, a.tile, l2);
		const int steps_mine = (l1 > 0 && e > s0) ? (int)(e - s0) : 0;
		int nsteps = steps_mine;
#pragma unroll
		for (int d = 32; d >= 1; d >>= 1) nsteps = imax(nsteps, __shfl_xor(nsteps, d));
		nsteps = uni(nsteps);
		const uint32_t *rw = r + (s0 >> 4);            /* (s0 is a multiple of 16) */
		const int nwords_mine = (steps_mine + 15) >> 4;
		uint32_t nxt = nwords_mine > 0 ? rw[0] : 0u;   /* the sixteen codes behind the ones in use */
		int d = l1, best = l1, best_t = 0;             /* D(l1, s0 + t), its minimum so far and the first t that has it */
		/* HITS: my own columns are s0 + t for own_lo < t <= steps_mine; the column in front of them is a warm-up column (or column 0) */
		const int own_lo = HITS ? (int)(n * a.tile - s0) : 0;
		const int hits_c = HITS ? scan_exact_bound(l1, a.use_cutoff, a.cutoff) : 0;
		bool run_on = false;                           /* HITS: inside a run of descents; its first and its latest value */
		int run_head = 0, run_tail = 0;
		/* the record of a run that ends in column `col`: a slot from the counter, the store only while the slot exists */
		auto append = [&](long long col, int tail, int head) {
			const unsigned long long slot = atomicAdd(a.cand_n, 1ull);
			if (slot < (unsigned long long)a.cand_cap) {
				a.cand_key[slot] = scan_cand_key(p, col);
				a.cand_val[slot] = scan_cand_val(tail, head);
			}
		};
		for (int tw = 0; tw * 16 < nsteps; ++tw) {
			uint32_t cw = nxt;
			nxt = tw + 1 < nwords_mine ? rw[tw + 1] : 0u;
#pragma unroll kColsUnrolled
			for (int cc = 0; cc < 16; ++cc) {
				const uint32_t c = cw;
				cw >>= 2;
				uint32_t pP = 0u, pM = 0u;                     /* the border row: D(0,j) - D(0,j-1) = 0 */
				const uint32_t nC0 = (c & 1u) - 1u, nC1 = ((c >> 1) & 1u) - 1u;   /* ~(bit of the code spread over the word) */
#pragma unroll
				for (int w = 0; w < W; ++w) {
					const uint32_t Eq = (B0[w] ^ nC0) & (B1[w] ^ nC1);
					const uint32_t Eqh = scan_or3<PAD_S>(Eq, pad[w], pM >> 31);   /* a wildcard row, or hin < 0 */
					const uint32_t sum = (Eqh & Pv[w]) + Pv[w];
					const uint32_t Xh = (sum ^ Pv[w]) | Eqh;
					const uint32_t Ph = Mv[w] | ~(Xh | Pv[w]);
					const uint32_t Mh = Pv[w] & Xh;
					const uint32_t Phs = __builtin_amdgcn_alignbit(Ph, pP, 31);   /* (Ph << 1) | hin > 0 */
					const uint32_t Mhs = __builtin_amdgcn_alignbit(Mh, pM, 31);
					const uint32_t Xv = scan_or3<PAD_S>(Eq, pad[w], Mv[w]);
					Pv[w] = Mhs | ~(Xv | Phs);
					Mv[w] = Phs & Xv;
					pP = Ph; pM = Mh;
					/* (HITS: left alone, the compiler sinks the Pv / Mv updates of all W words behind the candidate branch and keeps three
					 * temporaries per word alive across it -- 120 VGPRs at 16 words, 248 at 32; pinned here they are made where they stand) */
					if constexpr (HITS) asm volatile("" : "+v"(Pv[w]), "+v"(Mv[w]));
				}
				/* the last word's horizontal difference in its last row = D(l1, column) - D(l1, column - 1); behind my own tile the
				 * lane steps on over whatever the word held and keeps what it had */
				const int t1 = tw * 16 + cc + 1;
				d += (int)(pP >> 31) - (int)(pM >> 31);
				if constexpr (HITS) {
					/* a qualifying descent: own column, at or under c.  Consecutive ones are one RUN, and a run is one candidate record,
					 * appended in the first column behind it (rarely true: the skipped block holds the atomic and the stores) */
					const bool q = (pM >> 31) && d <= hits_c && t1 > own_lo && t1 <= steps_mine;
					if (run_on && !q) append(s0 + t1 - 1, run_tail, run_head);
					run_head = q && !run_on ? d : run_head;
					run_tail = q ? d : run_tail;
					run_on = q;
				} else {
					if (d < best && t1 <= steps_mine) { best = d; best_t = t1; }
				}
			}
		}
		if constexpr (HITS) {
			if (run_on) append(s0 + steps_mine, run_tail, run_head);   /* (a run up to my last column, which was the wave's last step) */
		} else {
			/* ---- the group's minimum of (score, absolute column), folded into the pair's slot ---- */
			unsigned long long key = steps_mine > 0 ? ((unsigned long long)(unsigned)best << 32) | (unsigned long long)(s0 + best_t) : ~0ull;
#pragma unroll
			for (int x = 32; x >= 1; x >>= 1) {
				const unsigned long long o = __shfl_xor(key, x, 64);
				key = o < key ? o : key;
			}
			if (lane == 0 && key != ~0ull) atomicMin(a.key + p, key);
		}
	}
}

__global__ __launch_bounds__(256) void at_scan_init_k(const ScanArgs a)
{
	const long long stride = (long long)gridDim.x * blockDim.x;
	for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < a.npairs; p += stride) {
		const long long qi = (a.s0 + p) / a.ntb;
		const int l1 = a.slen[scan_query_read(a.qperm[a.qa + qi], a.enc, a.nrev0)];
		a.key[p] = (unsigned long long)(unsigned)l1 << 32;     /* the candidate (l1, 0) */
	}
}

__global__ __launch_bounds__(256) void at_scan_unpack_k(const ScanArgs a)
{
	const long long stride = (long long)gridDim.x * blockDim.x;
	for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < a.npairs; p += stride) {
		const long long qi = (a.s0 + p) / a.ntb;
		const unsigned long long key = a.key[p];
		a.score[p] = (int)(unsigned)(key >> 32);
		a.end_i[p] = a.slen[scan_query_read(a.qperm[a.qa + qi], a.enc, a.nrev0)];
		a.end_j[p] = (int)(unsigned)key;
		a.state[p] = AT_ST_MID;
	}
}

/* a list entry's hit: (score, strand, target) of its key (at_search.hip.h); false for an empty entry */
AT_DEV bool scan_hit(unsigned long long key, int enc, int &score, int &strand, int &target)
{
	if (!key) return false;
	score = -(int)((unsigned)(key >> 32) ^ 0x80000000u);
	const unsigned low = ~(unsigned)key;
	target = (int)(low >> enc);
	strand = enc ? (int)(low & 1u) : 0;
	return true;
}

__global__ __launch_bounds__(256) void at_scan_window_k(const ScanWindowArgs a)
{
	const long long stride = (long long)gridDim.x * blockDim.x;
	for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < a.n; e += stride) {
		int score, strand, target;
		if (!scan_hit(a.lkey[e], a.enc, score, strand, target)) {
			a.woff1[e] = 0; a.woff2[e] = 0; a.len1[e] = 0; a.len2[e] = 0; a.ws[e] = 0;   /* an empty pair: no ops, no runs */
			continue;
		}
		const int q = a.eq ? a.eq[e] : (int)(e / a.k), qr = strand ? a.nrev0 + q : q, l1 = a.slen[qr], ej = a.lej[e];
		const int ws = (int)scan_window_start(ej, l1, score);
		a.woff1[e] = a.swoff[qr]; a.len1[e] = l1;
		a.woff2[e] = a.swoff[a.nq + target] + (ws >> 4); a.len2[e] = ej - ws;
		a.ws[e] = ws;
	}
}

__global__ __launch_bounds__(256) void at_scan_check_k(const ScanWindowArgs a)
{
	const long long stride = (long long)gridDim.x * blockDim.x;
	for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < a.n; e += stride) {
		int score, strand, target;
		if (!scan_hit(a.lkey[e], a.enc, score, strand, target)) {
			a.ncigar_out[e] = 0;
			for (int x = 0; x < 8; ++x) a.stats[e * 8 + x] = -1;
			continue;
		}
		const int nc = a.ncigar[e];
		if (a.w_score[e] != score || a.w_end_j[e] != a.lej[e] - a.ws[e] || nc < 0) *a.bad = 1;
		else a.stats[e * 8 + AT_CG_START_J] += a.ws[e];
		a.ncigar_out[e] = nc;
	}
}

}   // namespace at

template <bool HITS>
static const void *scan_kernel_of(int w)
{
	return w == 2 ? (const void *)at::at_scan<2, HITS> : w == 3 ? (const void *)at::at_scan<3, HITS> : w == 4 ? (const void *)at::at_scan<4, HITS>
	     : w == 5 ? (const void *)at::at_scan<5, HITS> : w == 8 ? (const void *)at::at_scan<8, HITS> : w == 16 ? (const void *)at::at_scan<16, HITS>
	     : w == 32 ? (const void *)at::at_scan<32, HITS> : nullptr;
}

extern "C" const void *at_scan_kernel(int w) { return scan_kernel_of<false>(w); }
extern "C" const void *at_scan_hits_kernel(int w) { return scan_kernel_of<true>(w); }

static hipError_t scan_launch_fn(const void *k, const at::ScanArgs *a, unsigned grid, hipStream_t s)
{
	void (*fn)(const at::ScanArgs) = (void (*)(const at::ScanArgs))k;
	if (!fn) return hipErrorInvalidValue;
	hipLaunchKernelGGL(fn, dim3(grid), dim3(64), 0, s, *a);
	return hipGetLastError();
}

extern "C" hipError_t at_scan_launch(const at::ScanArgs *a, int w, unsigned grid, hipStream_t s) { return scan_launch_fn(at_scan_kernel(w), a, grid, s); }

extern "C" hipError_t at_scan_hits_launch(const at::ScanArgs *a, int w, unsigned grid, hipStream_t s)
{
	if (!a->cand_n || a->cand_cap < 0 || (a->cand_cap > 0 && (!a->cand_key || !a->cand_val))) return hipErrorInvalidValue;
	return scan_launch_fn(at_scan_hits_kernel(w), a, grid, s);
}

static unsigned scan_small_grid(long long n, int ncu) { return (unsigned)std::max<long long>(1, std::min<long long>((n + 255) / 256, 8LL * ncu)); }

extern "C" hipError_t at_scan_init_launch(const at::ScanArgs *a, int ncu, hipStream_t s)
{
	hipLaunchKernelGGL(at::at_scan_init_k, dim3(scan_small_grid(a->npairs, ncu)), dim3(256), 0, s, *a);
	return hipGetLastError();
}

extern "C" hipError_t at_scan_unpack_launch(const at::ScanArgs *a, int ncu, hipStream_t s)
{
	hipLaunchKernelGGL(at::at_scan_unpack_k, dim3(scan_small_grid(a->npairs, ncu)), dim3(256), 0, s, *a);
	return hipGetLastError();
}

extern "C" hipError_t at_scan_window_launch(const at::ScanWindowArgs *a, int ncu, hipStream_t s)
{
	hipLaunchKernelGGL(at::at_scan_window_k, dim3(scan_small_grid(a->n, ncu)), dim3(256), 0, s, *a);
	return hipGetLastError();
}

extern "C" hipError_t at_scan_check_launch(const at::ScanWindowArgs *a, int ncu, hipStream_t s)
{
	hipLaunchKernelGGL(at::at_scan_check_k, dim3(scan_small_grid(a->n, ncu)), dim3(256), 0, s, *a);
	return hipGetLastError();
}
