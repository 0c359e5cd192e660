/*
 * at_queryplan.h -- the host arithmetic that the query-vs-target entries share (at_search, at_scan, at_scan_local, at_scan_fit,
 * at_scan_hits, at_allpairs_hits): the order in which the queries are swept and its blocks of one length, the bound
 * of a slice, the 64-bit key of a list entry, the pieces of a window pass, the CIGAR words that fit the caller's array and the tiles
 * of a block of the tiled scans.  Pure arithmetic: plain C++17, no HIP.
 *
 * The queries are swept in the stable order of their lengths.  With a reverse strand an entry of that order is (query << 1) | strand
 * (at_search.hip.h); with both strands a query's two entries are adjacent, strand 0 first: same length, same block, one run of
 * candidates for the merge.  A BLOCK is the run of entries of one length; its pairs with the targets go in SLICES.
 *
 * A list entry's key is (rank ^ 2^31) << 32 | ~low, low = target, or (target << 1) | strand with a reverse strand; rank is the score,
 * for distances its negative.  Unsigned key order is the ranking: higher rank first, then smaller target, then strand 0; 0 is the
 * empty slot (no entry has it: rank > INT32_MIN).  The device headers have their own copies of this arithmetic.
 */
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "at_localscan_plan.h"

namespace at {

constexpr int64_t kSliceDefault = 4LL << 20;   /* pairs of a slice when AT_ALLPAIRS_CHUNK says nothing */
constexpr int64_t kSliceMost = 1LL << 28;

struct QueryBlock { int qa, nqb; int32_t l1; };   /* the entries [qa, qa + nqb) of the order: queries of l1 bases */

struct QueryOrder {
	int enc = 0, two = 0;            /* entries carry a strand bit; every query has two entries */
	int64_t nv = 0;                  /* entries: nq << two */
	std::vector<int> qs, qperm;      /* the queries by length (stable); the entries */
	std::vector<QueryBlock> blocks;
};

/* strands: AT_STRAND_FWD / REV / BOTH = 1 / 2 / 3 (include/aligntools_hip.h) */
inline QueryOrder query_order(int64_t nq, const int32_t *q_len, int strands)
{
	QueryOrder o;
	o.enc = strands != 1; o.two = strands == 3;
	o.nv = nq << o.two;
	o.qs.resize((size_t)nq); o.qperm.resize((size_t)o.nv);
	for (int64_t q = 0; q < nq; ++q) o.qs[(size_t)q] = (int)q;
	std::stable_sort(o.qs.begin(), o.qs.end(), [&](int a, int b) { return q_len[a] < q_len[b]; });
	for (int64_t q = 0; q < nq; ++q) {
		const int c = o.qs[(size_t)q];
		if (o.two) { o.qperm[(size_t)(2 * q)] = c << 1; o.qperm[(size_t)(2 * q + 1)] = (c << 1) | 1; }
		else o.qperm[(size_t)q] = o.enc ? (c << 1) | 1 : c;
	}
	for (int64_t a = 0, b; a < nq; a = b) {
		const int32_t L = q_len[o.qs[(size_t)a]];
		for (b = a; b < nq && q_len[o.qs[(size_t)b]] == L; ++b) {}
		o.blocks.push_back({(int)(a << o.two), (int)((b - a) << o.two), L});
	}
	return o;
}

/* pairs of a slice: what the caller or AT_ALLPAIRS_CHUNK wants, at least 1, no more than the largest block has (`most`) or 2^28 */
constexpr int64_t slice_clamp(int64_t wanted, int64_t most)
{
	return std::max<int64_t>(1, std::min<int64_t>(wanted, std::min<int64_t>(std::max<int64_t>(most, 1), kSliceMost)));
}

struct ListKey { int32_t rank, target, strand; };

constexpr uint64_t list_key(int32_t rank, int32_t target, int strand, int enc)
{
	return ((uint64_t)((uint32_t)rank ^ 0x80000000u) << 32) | (uint32_t)~(enc ? ((uint32_t)target << 1) | (uint32_t)strand : (uint32_t)target);
}

constexpr ListKey list_key_decode(uint64_t key, int enc)
{
	const uint32_t low = ~(uint32_t)key;
	return {(int32_t)((uint32_t)(key >> 32) ^ 0x80000000u), (int32_t)(low >> enc), enc ? (int32_t)(low & 1u) : 0};
}

/* end of the piece of hits that starts at `a` (of n): at most hit_cap hits whose op slots, need(hit) bytes each, stay within
 * ops_cap -- but one hit at least, whatever it needs; *ops: the slots' sum */
template <typename Need>
inline int64_t piece_end(int64_t a, int64_t n, int64_t hit_cap, int64_t ops_cap, Need need, int64_t *ops = nullptr)
{
	int64_t sum = 0, b = a;
	for (; b < n && b - a < hit_cap; ++b) {
		const int64_t one = need(b);
		if (b > a && sum + one > ops_cap) break;
		sum += one;
	}
	if (ops) *ops = sum;
	return b;
}

/* off[0 .. n]: where the entries' words start in the device buffer; the words of the leading entries that end within `cap` */
inline int64_t prefix_fit(const int64_t *off, int64_t n, int64_t cap)
{
	int64_t fit = 0;
	for (int64_t e = 0; e < n && off[e + 1] <= cap; ++e) fit = off[e + 1];
	return fit;
}

/* The tiles of one block of a tiled scan (at_scan_local, at_scan_fit; at_localscan_plan.h has the cut, which is fit's too for targets
 * no shorter than the query -- a fit block has no others): the targets t_len[0 .. ntb), tiles of `tile` own columns and `ov` in front.
 * tpre[0] / tpre[1], [ntb + 1]: the swept tiles of the full shape (tile + ov columns) / the shorter ones at the targets' ends, of the
 * targets in front of target t. */
struct BlockTiles {
	int64_t tiles;       /* swept tiles of all targets, both passes */
	int32_t rag_most;    /* columns of the longest tile of the second pass; 0 without one */
};

inline BlockTiles block_tiles(const int32_t *t_len, int64_t ntb, int32_t tile, int64_t ov, std::vector<long long> tpre[2])
{
	BlockTiles b = {0, 0};
	for (int x = 0; x < 2; ++x) tpre[x].assign((size_t)ntb + 1, 0);
	for (int64_t t = 0; t < ntb; ++t) {
		const int32_t l2 = t_len[t];
		/* (the swept tiles: the repeats of tile 0 are left out) */
		const int64_t n = localscan_swept(l2, tile, ov), nf = localscan_swept_full(l2, tile, ov), d = localscan_dropped(l2, tile, ov);
		tpre[0][(size_t)t + 1] = tpre[0][(size_t)t] + nf;
		tpre[1][(size_t)t + 1] = tpre[1][(size_t)t] + (n - nf);
		for (int64_t k = nf; k < n; ++k) {
			const int64_t x = localscan_swept_tile(k, d);
			b.rag_most = std::max<int32_t>(b.rag_most, (int32_t)(localscan_tile_end(x, tile, ov, l2) - localscan_tile_start(x, tile, ov)));
		}
	}
	b.tiles = tpre[0][(size_t)ntb] + tpre[1][(size_t)ntb];
	return b;
}

}  // namespace at
