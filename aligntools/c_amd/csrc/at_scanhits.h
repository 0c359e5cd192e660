/*
 * at_scanhits.h -- the selection rule of at_scan_hits: which candidates of a sweep are occurrences, which
 * occurrences a separation keeps, and the order of a query's hits.  Pure arithmetic: plain C++17, no HIP; the marking kernel
 * (at_scanhits.hip) and the host's finishing step share it, and tests/c/scanhits_check.cpp checks it against the definition.
 *
 * A DESCENT of the last row at or under the bound is a column j >= 1 with D(l1,j) <= c and D(l1,j) < D(l1,j-1), c = min(max_dist,
 * l1 - 1).  A CANDIDATE record is a run of descents in consecutive columns (a sweep cuts runs where it likes -- at its tile borders --
 * and may leave every descent a run of its own): key = (pair << 32) | the run's LAST column, pair being the slice's index of the
 * (query entry, target) -- a (query, strand, target) triple --, val = the run's last value (TAIL, the one that can be an occurrence:
 * every other descent of a run is followed by a lower one) and its first value (HEAD, what the descent in front of the run sees
 * next).  The candidates of a slice are sorted by key, so that a pair's candidates are consecutive and in column order.
 *   valley      candidate i is an OCCURRENCE (column, tail) iff it is its pair's last candidate or the next one's head is not below
 *               its tail: the next descent after a plateau that ends in a rise can only be as low again; after one that ends in a
 *               fall it IS that fall
 *   separation  an occurrence (a, v) is KEPT iff no other occurrence (a', v') of its pair with |a - a'| <= sep has
 *               (v', a') < (v, a); sep = 0 keeps all.  A window minimum, not a chain: the result has no processing order
 *   order       a query's hits by (distance, target, strand, column)
 */
#pragma once
#include <algorithm>
#include <cstdint>

#if defined(__HIPCC__)
#define AT_SH_FN __host__ __device__ inline
#else
#define AT_SH_FN inline
#endif

#ifndef AT_SCAN_SEP_READ
#define AT_SCAN_SEP_READ (-1)   /* (include/aligntools_hip.h) min_sep: each query's own length */
#endif

namespace at {

constexpr long long kScanHitsDefaultCand = 1LL << 20;   /* candidate records of a slice when the caller names no capacity */

struct ScanHit {
	int32_t query, target, strand, score, end_j;
};

/* c: a match must cost less than deleting the whole read (l1 >= 1) */
constexpr int32_t scan_hits_bound(int32_t l1, int32_t max_dist) { return max_dist < l1 - 1 ? max_dist : l1 - 1; }

/* the separation of a query of l1 bases */
constexpr int64_t scan_hits_sep(int32_t min_sep, int32_t l1) { return min_sep == AT_SCAN_SEP_READ ? l1 : min_sep; }

AT_SH_FN uint64_t scan_cand_key(int64_t pair, int64_t column) { return ((uint64_t)pair << 32) | (uint64_t)(uint32_t)column; }
AT_SH_FN int64_t scan_cand_pair(uint64_t key) { return (int64_t)(key >> 32); }
AT_SH_FN int64_t scan_cand_column(uint64_t key) { return (int64_t)(uint32_t)key; }
/* (distances are at most kScanMaxQuery: sixteen bits each) */
AT_SH_FN int32_t scan_cand_val(int32_t tail, int32_t head) { return (int32_t)((uint32_t)tail | ((uint32_t)head << 16)); }
AT_SH_FN int32_t scan_cand_tail(int32_t val) { return (int32_t)((uint32_t)val & 0xffffu); }
AT_SH_FN int32_t scan_cand_head(int32_t val) { return (int32_t)((uint32_t)val >> 16); }

/* candidate i of the n sorted ones is an occurrence */
AT_SH_FN bool scan_is_valley(const uint64_t *key, const int32_t *val, int64_t n, int64_t i)
{
	return i + 1 >= n || scan_cand_pair(key[i + 1]) != scan_cand_pair(key[i]) || scan_cand_head(val[i + 1]) >= scan_cand_tail(val[i]);
}

/* candidate i is an occurrence that the separation sep >= 0 keeps */
AT_SH_FN bool scan_hit_kept(const uint64_t *key, const int32_t *val, int64_t n, int64_t i, int64_t sep)
{
	if (!scan_is_valley(key, val, n, i)) return false;
	const int64_t p = scan_cand_pair(key[i]), a = scan_cand_column(key[i]);
	const int32_t v = scan_cand_tail(val[i]);
	/* an earlier occurrence wins a tie on the value, a later one must be strictly lower */
	for (int64_t x = i - 1; x >= 0 && scan_cand_pair(key[x]) == p && a - scan_cand_column(key[x]) <= sep; --x)
		if (scan_cand_tail(val[x]) <= v && scan_is_valley(key, val, n, x)) return false;
	for (int64_t x = i + 1; x < n && scan_cand_pair(key[x]) == p && scan_cand_column(key[x]) - a <= sep; ++x)
		if (scan_cand_tail(val[x]) < v && scan_is_valley(key, val, n, x)) return false;
	return true;
}

/* the order of the hits: by query, and a query's hits by (distance, target, strand, column) */
AT_SH_FN bool scan_hit_less(const ScanHit &x, const ScanHit &y)
{
	if (x.query != y.query) return x.query < y.query;
	if (x.score != y.score) return x.score < y.score;
	if (x.target != y.target) return x.target < y.target;
	if (x.strand != y.strand) return x.strand < y.strand;
	return x.end_j < y.end_j;
}

inline void scan_hits_order(ScanHit *hits, int64_t n) { std::sort(hits, hits + n, scan_hit_less); }

}  // namespace at
