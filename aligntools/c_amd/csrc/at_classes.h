/*
 * at_classes.h -- the row classes of the packed kernels, once: a read of l1 bases takes the first class of its
 * family whose g lanes x k rows hold it, and the instantiation units hold a kernel for every class named here.  Plain C++17, no HIP.
 */
#pragma once
#include "../../../include/aligntools_hip.h"

#include <cstddef>

namespace at {

struct RowClass { int max_l1, k; };   /* reads of up to max_l1 bases: k rows per lane */

/* one strip of g lanes x k rows per class (g * k >= max_l1) */
constexpr RowClass kClass4[] = {{36, 9}, {40, 10}, {52, 13}, {64, 16}, {76, 19}};                                        /* uniform batches only */
constexpr RowClass kClass8[] = {{40, 5}, {48, 6}, {56, 7}, {64, 8}, {80, 10}, {104, 13}, {128, 16}, {152, 19}};
constexpr RowClass kClass16[] = {{64, 4}, {80, 5}, {96, 6}, {112, 7}, {160, 10}, {208, 13}, {256, 16}, {304, 19}};
constexpr RowClass kClass32[] = {{224, 7}, {256, 8}, {320, 10}, {384, 12}, {416, 13}, {512, 16}, {608, 19}};
constexpr size_t kClass32RagFirst = 2;   /* ragged frames and force_g == 32: from 10 rows up, whatever l1 is */
constexpr int kClass32SkipUnderGroup32 = 12;   /* AT_GROUP=32 (the round-1 classes): no 12-row class */
/* ragged packed overlap with tracebacks: the 64-lane group, strips of 256 rows up to 256 bases, one strip of 1 024 beyond */
constexpr RowClass kClassOvl[] = {{256, 4}, {1024, 16}};
/* the bit-parallel kernels' words per lane: one alignment per lane (32 rows per word), and one per 32 lanes (1 024 rows per word) */
constexpr RowClass kMyersLaneWords[] = {{64, 2}, {96, 3}, {128, 4}, {160, 5}, {256, 8}, {512, 16}, {1024, 32}};
constexpr RowClass kMyersGroupWords[] = {{1024, 1}, {2048, 2}, {4096, 4}, {8192, 8}, {16384, 16}, {32768, 32}};

/* k of the first class from t[first] on that holds l1 (and is not skip_k); the last class for anything longer */
template <size_t N>
constexpr int class_rows(const RowClass (&t)[N], int l1, size_t first = 0, int skip_k = 0)
{
	for (size_t q = first; q + 1 < N; ++q)
		if (l1 <= t[q].max_l1 && t[q].k != skip_k) return t[q].k;
	return t[N - 1].k;
}
template <size_t N>
constexpr int class_top(const RowClass (&t)[N]) { return t[N - 1].max_l1; }

/* the longest read with a one-strip frame: 32 lanes x 19 rows for local, x 16 for global, x 13 for fit (the others spill there and
 * lose to the strips of the 64-lane group); overlap: 64 lanes x 16 rows */
constexpr int kTopLocal = 608, kTopGlobal = 512, kTopFit = 416, kTopOverlap = class_top(kClassOvl);
constexpr int one_strip_top(int mode)
{
	return mode == AT_MODE_LOCAL ? kTopLocal : mode == AT_MODE_GLOBAL ? kTopGlobal : mode == AT_MODE_FIT ? kTopFit : kTopOverlap;
}

/* the longest read of a ragged frame per group width */
constexpr int kRagGroups[] = {8, 16, 32, 64};
constexpr int rag_group_top(int g)
{
	return g == 8 ? class_top(kClass8) : g == 16 ? class_top(kClass16) : g == 32 ? class_top(kClass32) : kTopOverlap;
}

/* (group width, rows per lane) of a read in a ragged batch.  Local frames mix read lengths freely and run on the 16-lane groups up to
 * 304 bases (on the 8-lane groups, whose lanes carry up to 19 rows, the same batches ran 15 % slower: 100..150 x 100..150 2.9
 * against 2.5 ms per 100k pairs), on the 32-lane groups beyond; global / fit: 8-lane groups up to 152 bases, 16-lane up to
 * 304, 32-lane beyond; overlap with tracebacks: the 64-lane group */
struct GroupRows { int g, k; };
constexpr bool operator==(const GroupRows &a, const GroupRows &b) { return a.g == b.g && a.k == b.k; }
constexpr bool operator!=(const GroupRows &a, const GroupRows &b) { return !(a == b); }
constexpr GroupRows rag_class(int mode, bool overlap_tb, int l1)
{
	if (mode == AT_MODE_OVERLAP && overlap_tb) return {64, class_rows(kClassOvl, l1)};
	if (l1 > class_top(kClass16)) return {32, class_rows(kClass32, l1, kClass32RagFirst)};
	if (mode == AT_MODE_LOCAL || l1 > class_top(kClass8)) return {16, class_rows(kClass16, l1)};
	return {8, class_rows(kClass8, l1)};
}

/* bytes of LDS for the s2 windows of the n alignments of a bit-parallel wavefront (16 bases per word, odd stride, as the kernels compute it) */
constexpr size_t myers_window_bytes(int n, int max_l2) { return (size_t)n * ((((size_t)max_l2 + 15) / 16 + 2) | 1) * 4; }

}  // namespace at
