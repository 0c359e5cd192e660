/*
 * at_cigar.hip.h -- run-length CIGARs and alignment statistics made on the device (at_cigar.hip) from what the sweep kernels leave
 * in HBM: the op codes of a traceback in END -> START order, the cell it started from and the packed sequences.
 *
 * A column's class is a BAM op code of "MIDNSHP=X": AT_OP_MID with equal bytes '=' (7), with unequal bytes 'X' (8), AT_OP_LOW 'I' (1),
 * AT_OP_UPP 'D' (2), AT_OP_JUMP 'N' (3); with `merge` (AT_CIGAR_M) '=' and 'X' are both 'M' (0).  A word is (run length << 4) | code,
 * words in reading order (START -> END).
 *
 * W lanes per pair, 64 / W pairs side by side in a wavefront, passes of W ops as at_render_k: the row / column an op consumes is
 * the end cell minus a prefix count (ballot + popcount).  A lane is the head of a run if its class differs from that of the op
 * before it (the lane below, by a shuffle inside the group; lane 0: the class carried over from the pass before); one ballot of
 * the heads gives every run its number (counted from the END) and its length (the distance to the next head).  The run that is
 * still open at the end of a pass is carried (class, length so far) into the next one; it is written by the head that closes it,
 * the last run of a list by lane 0 behind the last pass.
 *
 * Two phases around the scan of the counts (at_scan_tiles / at_scan_nops, "sizes first, then one payload"):
 *   phase 0  ncigar[k] = runs, stats[k][0..7] = start_i, start_j, equal, unequal, I bases, D bases, N bases, I runs + D runs;
 *            a pair the sweep refused (nops < 0) or whose list is inconsistent (a code above 3, a walk below row / column 0 --
 *            checked before the load) gets ncigar = -1 and a row of -1
 *   phase 1  run r (from the END) of pair k goes to cigar[cigar_off[k] + ncigar[k] - 1 - r]; pairs with ncigar <= 0 and pairs that
 *            would end beyond `cap` are skipped whole
 */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace at {

struct CigarArgs {
	long long npairs;
	const uint32_t *seq;
	const long long *woff1, *woff2;
	const int *end_i, *end_j;
	const uint8_t *ops;
	const long long *ops_off;
	const int *nops;
	int merge;                     /* '=' and 'X' become 'M' */
	int *ncigar;                   /* phase 0 writes, phase 1 reads */
	int *stats;                    /* [npairs][8], may be NULL */
	const long long *cigar_off;    /* phase 1: exclusive scan of max(ncigar, 0) */
	uint32_t *cigar;
	long long cap;                 /* words in cigar */
};

}   // namespace at

/* at_cigar.hip: the launch of one phase (asynchronous on s; returns the launch's error).  bits 2 / 8, w 16 / 64 lanes per pair */
extern "C" hipError_t at_cigar_launch(const at::CigarArgs *a, int bits, int w, int phase, int ncu, hipStream_t s);
