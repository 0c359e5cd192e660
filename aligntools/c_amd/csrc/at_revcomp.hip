/* at_revcomp.hip -- the reverse-complement kernel for packed reads and its launch (at_revcomp.hip.h) */
#include "at_revcomp.hip.h"

#include <algorithm>

namespace at {

__constant__ CompTable d_comp = make_comp_table();

template <int BITS>
__global__ __launch_bounds__(256) void at_revcomp_k(const RevcompArgs a)
{
	constexpr int BPW = 32 / BITS, LOG = BITS == 2 ? 4 : 2;
	const int l16 = threadIdx.x & 15;
	const long long first = (long long)blockIdx.x * 16 + (threadIdx.x >> 4);
	const long long stride = (long long)gridDim.x * 16;
	for (long long s = first; s < a.nseq; s += stride) {
		const uint32_t *src = a.seq + a.woff[s];
		const int len = a.len[s];
		uint32_t *dst = a.out + a.out_woff[s];
		const int nw = (len + BPW - 1) / BPW + 1;        /* the zero slack word included */
		for (int w = l16; w < nw; w += 16) {
			uint32_t v = 0;
			const int cnt = len - w * BPW;                /* bases of this word and beyond */
			if (cnt > 0) {
				/* the window: forward bases sb .. sb + BPW - 1, sb = len - BPW (w + 1) > -BPW; bases below 0 read as zero */
				const int sb = cnt - BPW;
				const int wlo = sb >> LOG;                /* (arithmetic shift: -1 for sb < 0) */
				const unsigned sh = (unsigned)(sb & (BPW - 1)) * BITS;
				const uint32_t lo = wlo >= 0 ? src[wlo] : 0u;
				const uint32_t hi = sh ? src[wlo + 1] : 0u;   /* (the word of base len - 1 - BPW w: inside the read) */
				uint32_t x = __builtin_amdgcn_alignbit(hi, lo, sh);
				if constexpr (BITS == 2) {
					x = __builtin_bitreverse32(x);                                /* fields reversed, the bits of each swapped */
					x = ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1);
					v = ~x;                                                       /* A0 C1 G2 T3: the complement is code ^ 3 */
					if (cnt < BPW) v &= (1u << (2 * cnt)) - 1u;
				} else {
					x = __builtin_amdgcn_perm(0u, x, 0x00010203u);                /* bytes reversed */
					v = (uint32_t)d_comp.t[x & 255u] | (uint32_t)d_comp.t[(x >> 8) & 255u] << 8 |
					    (uint32_t)d_comp.t[(x >> 16) & 255u] << 16 | (uint32_t)d_comp.t[x >> 24] << 24;
					if (cnt < BPW) v &= (1u << (8 * cnt)) - 1u;
				}
			}
			dst[w] = v;
		}
	}
}

}   // namespace at

extern "C" hipError_t at_revcomp_launch(const at::RevcompArgs *a, int bits, int ncu, hipStream_t s)
{
	if (a->nseq <= 0) return hipSuccess;
	const unsigned grid = (unsigned)std::max<long long>(1, std::min<long long>((a->nseq + 15) / 16, 8LL * ncu));
	if (bits == 2) hipLaunchKernelGGL(at::at_revcomp_k<2>, dim3(grid), dim3(256), 0, s, *a);
	else hipLaunchKernelGGL(at::at_revcomp_k<8>, dim3(grid), dim3(256), 0, s, *a);
	return hipGetLastError();
}
