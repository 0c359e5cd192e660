/*
 * at_infix.hip.h -- edit INFIX mode (at_set_edit_infix; kernels in at_infix.hip): the best match of a read inside a target, approximate
 * matching in Myers' original sense.  The rule is this library's (the reference's edit_dist, alignment.h:291-315, is global only):
 *   D(0,j) = 0, D(i,0) = i, D(i,j) = min(D(i,j-1) + 1, D(i-1,j-1) + (s1[i-1] != s2[j-1]), D(i-1,j) + 1)
 *   score = min over 0 <= j <= l2 of D(l1,j), end cell (l1, j*) with j* the SMALLEST j attaining it, state AT_ST_MID.
 * Ops (TB kernels) END -> START from (l1, j*) until i == 0; at (i, j) the first rule that holds:
 *   1. j > 0 && D(i-1,j-1) + (s1[i-1] != s2[j-1]) == D(i,j)   AT_OP_MID, i--, j--
 *   2. D(i-1,j) + 1 == D(i,j)                                 AT_OP_LOW, i--
 *   3. otherwise                                              AT_OP_UPP, j--
 * (at j == 0 rule 2 always holds); the walk ends in (0, j0), nops <= l1 + l2, mismatch columns + gap columns = score.
 *
 * Mapping: one alignment per lane, W words of 32 rows, as at_myers<W, 1> (at_myers.hip.h) -- 64 s2 windows in LDS at the odd stride,
 * one LDS word per sixteen columns, work from the device queue.
 *
 * Rows are BOTTOM-ALIGNED, as the overlap filter (SEMI) loads s1: row l1 is bit 31 of word W - 1, so D(l1,j) - D(l1,j-1) is the sign
 * pair the last word step leaves behind anyway (Ph >> 31, Mh >> 31) and capturing it costs nothing per word.  The pad = 32 W - l1
 * rows in front are WILDCARDS: they match every base (pad[w] is or-ed into the two places Eq is consumed, each of which stays one
 * three-input or) and their Pv starts at 0, so D is 0 on every pad row in every column and the pad IS the zero border D(0,j) = 0 of
 * the first real row.  The word step stays at the 14 instructions of at_myers; the top-aligned alternative (rows as in at_edit_tb,
 * the word that holds row l1 selected inside the unrolled loop) adds two selects per word (DESIGN.md 3.11 has the counts).
 * Per column the lane adds the sign pair to a running d (from l1) and keeps best / best_j under a strict <, while inside its OWN l2:
 * the lanes of a wave run to the longest l2.
 *
 * TB: after column j = 1 .. l2 the lane stores Pv[w] / Mv[w] into the wavefront's slab exactly as at_edit_tb does,
 * [column - 1][word][plane][lane], max_l2 * W * 512 bytes per wavefront; the same wavefront walks from (l1, j*).  The walk is
 * at_edit_tb's in PADDED row coordinates (row ip = pad + i; it stops at ip == pad): a column's value is 0 + the vertical differences
 * of the rows <= ip (the pad rows contribute 0, their words are skipped), and column 0 is ~pad (Pv = 1 on the real rows: D(i,0) = i).
 *
 * anchor_end (TB, at_scan_hits' windows only): the walk starts in (l1, l2) with the value the fill ended on instead of (l1, j*) -- an
 * occurrence that is not the best of its target is not the arg-min of its window either.
 *
 * The word step is repeated here from at_myers.hip.h, as at_edit_tb.hip repeats it: the committed counter files fingerprint
 * at_myers.hip.h, so folding the three copies into one belongs to a change that re-collects the counters.
 */
#pragma once
#include "at_myers.hip.h"

namespace at {

struct InfixArgs {
	MyersArgs m;                   /* the pairs, their results, the order and the work queue (no all-vs-all, no SEMI) */
	uint8_t *ops;                  /* TB: op codes END -> START, pair p at ops[ops_off[p] ..] */
	const long long *ops_off;
	uint32_t *slab;                /* TB: gridDim.x slabs of slab_words words */
	long long slab_words;          /* max_l2 * W * 128 */
	int anchor_end;                /* TB: the end cell is (l1, l2), not the arg-min of the last row (at_scan_hits; 0 everywhere else) */
};

}   // namespace at

typedef void (*at_infix_fn)(const at::InfixArgs);
/* at_infix.hip: the kernel for w words per lane, w in {2, 3, 4, 5, 8, 16, 32} (reads of up to 32 w bases), with (tb != 0) or without the
 * op lists, or nullptr */
at_infix_fn at_pick_infix(int w, int tb);
