/*
 * at_edit_tb.hip.h -- the alignment behind an edit distance (at_set_edit_traceback; kernel in at_edit_tb.hip): the bit-parallel fill of
 * at_myers<W, 1> (at_myers.hip.h: one alignment per lane, W words of 32 rows) that keeps every column's vertical differences, and a walk
 * over them by the same wavefront.
 *
 * The rule (ours: the reference's edit_dist, alignment.h:291-315, returns a number only).  D is edit_dist's table with u = 1:
 * D(i,0) = i, D(0,j) = j, D(i,j) = min(D(i,j-1) + 1, D(i-1,j-1) + (s1[i-1] != s2[j-1]), D(i-1,j) + 1).  The op list is emitted
 * END -> START from (l1, l2) to (0, 0); at (i, j) the first rule that holds:
 *   1. i > 0 && j > 0 && D(i-1,j-1) + (s1[i-1] != s2[j-1]) == D(i,j)   AT_OP_MID, i--, j--
 *   2. i > 0 && D(i-1,j) + 1 == D(i,j)                                 AT_OP_LOW, i--
 *   3. otherwise                                                       AT_OP_UPP, j--
 * score = D(l1,l2), end cell (l1,l2), state AT_ST_MID, nops <= l1 + l2; mismatch columns + gap columns = score.
 *
 * Fill.  After column j = 1 .. l2 an active lane stores Pv[w] / Mv[w] (bit r of word w: D(32w+r+1, j) - D(32w+r, j) = +1 / -1) into
 * the wavefront's slab, laid out [column - 1][word][plane][lane]: one store instruction of the wave is 256 contiguous bytes.  Column 0
 * (Pv all ones, Mv 0) is not stored.  A work item needs max_l2 * W * 512 slab bytes.
 *
 * Walk.  One walker per lane, straight behind the fill; a lane reads only words it stored itself.  It keeps A = D(i,j), B = D(i,j-1)
 * and the words of row i of the columns j and j - 1 (dv(i,j), dv(i,j-1): one bit each of Pv and Mv).  Rule 1 compares B - dv(i,j-1) +
 * mismatch with A; rule 2 is dv(i,j) == +1.  A step up: A -= dv(i,j), B -= dv(i,j-1).  A step into column j - 1: A from B (minus
 * dv(i,j-1) on the diagonal), B = (j-2) + sum over the words of rows <= i of popc(Pv) - popc(Mv) of column j - 2: at most W word
 * pairs per column move.  s1's bases come from its packed words, s2's from the LDS window the fill staged.
 */
#pragma once
#include "at_myers.hip.h"

namespace at {

struct EditTbArgs {
	MyersArgs m;                   /* the pairs, their results, the order and the work queue (no all-vs-all, no SEMI) */
	uint8_t *ops;                  /* op codes END -> START, pair p at ops[ops_off[p] ..] */
	const long long *ops_off;
	uint32_t *slab;                /* gridDim.x slabs of slab_words words */
	long long slab_words;          /* max_l2 * W * 128 */
};

}   // namespace at

typedef void (*at_edit_tb_fn)(const at::EditTbArgs);
/* at_edit_tb.hip: the kernel for w words per lane, w in {2, 3, 4, 5, 8, 16, 32} (reads of up to 32 w bases), or nullptr */
at_edit_tb_fn at_pick_edit_tb(int w);
