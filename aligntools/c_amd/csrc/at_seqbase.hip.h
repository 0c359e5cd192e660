/* at_seqbase.hip.h -- one base of a packed sequence as the byte the reference compares and prints: what the kernels that turn an op
 * list back into text or into CIGAR classes read (at_render.hip.h, at_cigar.hip) */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace at {

template <int BITS>
__device__ __forceinline__ uint32_t render_base(const uint32_t *seq, long long woff, int idx)
{
	if constexpr (BITS == 2) {
		const uint32_t w = seq[woff + (idx >> 4)];
		const uint32_t code = (w >> (2 * (idx & 15))) & 3u;
		return (0x54474341u >> (8 * code)) & 0xffu;            /* 0..3 -> 'A','C','G','T' */
	} else {
		const uint32_t w = seq[woff + (idx >> 2)];
		return (w >> (8 * (idx & 3))) & 0xffu;
	}
}

} /* namespace at */
