/*
 * at_revcomp.hip.h -- the reverse complement of PACKED reads, made on the device (at_revcomp.hip): what a both-strand search
 * (at_search_strands) and a caller of at_align_batch_device with device-resident reads need for the second strand.
 *
 * For each read the kernel reads its packed words and writes the packed words of its reverse complement, bit for bit what at_pack
 * produces for the reverse-complemented bytes: the same word count (ceil(len / bases per word) + the zero slack word), zero bits
 * behind the last base.  Sixteen lanes per read, one lane per output word and pass, as at_pack.
 *   2 bits: output word i holds forward bases len-1-16i down to len-16-16i: a 32-bit window over two neighbouring forward words
 *           (v_alignbit), the sixteen fields reversed (v_bfrev, then the two bits of each field swapped), XOR all ones (A<->T,
 *           C<->G is code ^ 3), masked to the bases the word holds.  Forward words before the read's first count as zero.
 *   8 bits: the same window over four bytes, the bytes reversed (v_perm) and mapped through the complement table that
 *           AT_COMPLEMENT_PAIRS (include/aligntools_hip.h) states: IUPAC in both letter cases, every other byte unchanged.
 */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aligntools_hip.h"

namespace at {

/* the complement of every byte value, from AT_COMPLEMENT_PAIRS (upper case; the lower-case letters follow) */
struct CompTable { uint8_t t[256]; };
constexpr CompTable make_comp_table()
{
	CompTable c{};
	for (int i = 0; i < 256; ++i) c.t[i] = (uint8_t)i;
	constexpr const char *p = AT_COMPLEMENT_PAIRS;
	for (int i = 0; p[i] && p[i + 1]; i += 2) {
		c.t[(uint8_t)p[i]] = (uint8_t)p[i + 1];
		c.t[(uint8_t)p[i] + 32] = (uint8_t)(p[i + 1] + 32);
	}
	return c;
}

struct RevcompArgs {
	long long nseq;
	const uint32_t *seq;           /* the forward reads' packed words */
	const long long *woff;         /* [nseq] word offset of read r in seq */
	const int *len;                /* [nseq] bases */
	uint32_t *out;
	const long long *out_woff;     /* [nseq] word offset of read r's reverse complement in out */
};

}   // namespace at

/* at_revcomp.hip: the launch (asynchronous on s; returns the launch's error) */
extern "C" hipError_t at_revcomp_launch(const at::RevcompArgs *a, int bits, int ncu, hipStream_t s);
