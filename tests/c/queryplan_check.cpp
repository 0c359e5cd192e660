/*
 * queryplan_check.cpp -- the host arithmetic of the query-vs-target entries (csrc/at_queryplan.h) without a GPU.  Built by `make asan`
 * with AddressSanitizer and UBSan and run by tests/test_queryplan_check.py.  The header is compared with a plain restatement of the
 * loops the entries had each for themselves (ref_* below), over seeded query sets of 0 .. 200 reads of few distinct lengths and all
 * three strand settings:
 *   1. qperm is a permutation of the encoded entries; the blocks partition [0, nv); within a block all lengths are equal and the
 *      caller's order is kept; with both strands a query's two entries are adjacent, strand 0 first;
 *   2. the slice clamp at most = 0, 1 and 2^28, beyond it, and with a wanted size below 1;
 *   3. list keys round-trip at the extremes of rank and target, and their order is the ranking;
 *   4. the piece cutter never returns an empty piece, respects both caps except for a single oversized hit, covers every hit once;
 *   5. the prefix fit at capacity 0, at exactly one entry's end, and when everything fits;
 *   6. a block's tile prefix arrays, tile count and longest ragged tile against the loops of the local and the fit scan, at query
 *      lengths 1 .. 1 024, tiles of 16, 64 and 1 024 columns, with and without a cutoff, over target lengths around every edge of the cut.
 * Exit status 0 and "queryplan_check: ok" when everything holds; every failure is printed.
 */
#include "../../aligntools/c_amd/csrc/at_queryplan.h"
#include "../../aligntools/c_amd/csrc/at_fitscan_plan.h"

#include <climits>
#include <cstdio>
#include <initializer_list>

static int g_failures = 0;
#define CHECK(cond, ...)                                                        \
	do {                                                                        \
		if (!(cond)) {                                                          \
			if (++g_failures <= 40) { printf("FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
		}                                                                       \
	} while (0)

static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd()
{
	g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17;
	return g_state;
}
static int64_t between(int64_t lo, int64_t hi) { return lo + (int64_t)(rnd() % (uint64_t)(hi - lo + 1)); }

/* ---- the loops as the entries had them ---- */
struct RefBlock { int qa, nqb; int32_t l1; };
static void ref_order(int64_t nq, const int32_t *q_len, int strands, std::vector<int> &qs, std::vector<int> &qperm, std::vector<RefBlock> &blocks)
{
	const int enc = strands != 1, two = strands == 3;
	const int64_t nv = nq << two;
	qs.assign((size_t)nq, 0); qperm.assign((size_t)nv, 0); blocks.clear();
	for (int64_t q = 0; q < nq; ++q) qs[(size_t)q] = (int)q;
	std::stable_sort(qs.begin(), qs.end(), [&](int a, int b) { return q_len[a] < q_len[b]; });
	for (int64_t q = 0; q < nq; ++q) {
		const int c = qs[(size_t)q];
		if (two) { qperm[(size_t)(2 * q)] = c << 1; qperm[(size_t)(2 * q + 1)] = (c << 1) | 1; }
		else qperm[(size_t)q] = enc ? (c << 1) | 1 : c;
	}
	for (int64_t a = 0, b; a < nq; a = b) {
		const int32_t L = q_len[qs[(size_t)a]];
		for (b = a; b < nq && q_len[qs[(size_t)b]] == L; ++b) {}
		blocks.push_back({(int)(a << two), (int)((b - a) << two), L});
	}
}

static int64_t ref_clamp(int64_t chunk, int64_t most)
{
	return std::max<int64_t>(1, std::min<int64_t>(chunk, std::min<int64_t>(std::max<int64_t>(most, 1), 1LL << 28)));
}

/* (the local scan said its bound in two steps) */
static int64_t ref_clamp_local(int64_t chunk, int64_t most_tiles)
{
	chunk = std::max<int64_t>(1, std::min<int64_t>(chunk, 1LL << 28));
	return std::min<int64_t>(chunk, std::max<int64_t>(most_tiles, 1));
}

static void check_order(int64_t nq, int strands, int nlengths)
{
	std::vector<int32_t> q_len((size_t)nq);
	for (auto &l : q_len) l = (int32_t)(between(0, nlengths - 1) * 37);
	const at::QueryOrder o = at::query_order(nq, q_len.data(), strands);
	std::vector<int> qs, qperm;
	std::vector<RefBlock> blocks;
	ref_order(nq, q_len.data(), strands, qs, qperm, blocks);
	const int enc = strands != 1, two = strands == 3;
	CHECK(o.enc == enc && o.two == two && o.nv == nq << two, "nq=%lld strands=%d", (long long)nq, strands);
	CHECK(o.qs == qs && o.qperm == qperm, "nq=%lld strands=%d: the order differs from the entries' loops", (long long)nq, strands);
	CHECK(o.blocks.size() == blocks.size(), "%zu blocks, %zu expected", o.blocks.size(), blocks.size());
	for (size_t x = 0; x < o.blocks.size() && x < blocks.size(); ++x)
		CHECK(o.blocks[x].qa == blocks[x].qa && o.blocks[x].nqb == blocks[x].nqb && o.blocks[x].l1 == blocks[x].l1, "block %zu", x);
	/* a permutation of the encoded entries */
	std::vector<int> seen((size_t)(nq << 1), 0);
	for (int v : o.qperm) {
		const int q = enc ? v >> 1 : v, strand = enc ? v & 1 : 0;
		CHECK(q >= 0 && q < nq, "entry %d names query %d of %lld", v, q, (long long)nq);
		if (q < 0 || q >= nq) return;
		CHECK(strands == 3 || strand == (strands == 2), "entry %d: strand %d under strands=%d", v, strand, strands);
		++seen[(size_t)(2 * q + strand)];
	}
	for (int64_t q = 0; q < nq; ++q)
		for (int st = 0; st < 2; ++st)
			CHECK(seen[(size_t)(2 * q + st)] == ((strands == 3 || st == (strands == 2)) ? 1 : 0), "query %lld strand %d seen %d times", (long long)q, st, seen[(size_t)(2 * q + st)]);
	/* the blocks partition [0, nv); equal lengths, caller order, rising lengths; both strands adjacent */
	int64_t at_entry = 0;
	int32_t last_len = -1;
	for (const at::QueryBlock &B : o.blocks) {
		CHECK(B.qa == at_entry && B.nqb > 0, "block starts at %d, expected %lld", B.qa, (long long)at_entry);
		CHECK(B.l1 > last_len, "block of length %d behind one of %d", B.l1, last_len);
		last_len = B.l1;
		int prev = -1;
		for (int x = B.qa; x < B.qa + B.nqb && x < (int)o.qperm.size(); ++x) {
			const int v = o.qperm[(size_t)x], q = enc ? v >> 1 : v;
			CHECK(q_len[(size_t)q] == B.l1, "entry %d of a block of %d has %d bases", x, B.l1, q_len[(size_t)q]);
			if (two) {
				CHECK((x & 1) == (v & 1) && (!(x & 1) || (o.qperm[(size_t)x - 1] >> 1) == q), "entry %d: strands of query %d not adjacent, forward first", x, q);
				if (!(x & 1)) { CHECK(q > prev, "caller order: %d behind %d", q, prev); prev = q; }
			} else { CHECK(q > prev, "caller order: %d behind %d", q, prev); prev = q; }
		}
		at_entry += B.nqb;
	}
	CHECK(at_entry == o.nv, "blocks cover %lld of %lld entries", (long long)at_entry, (long long)o.nv);
}

static void check_clamp()
{
	const int64_t wanted[] = {LLONG_MIN, -5, 0, 1, 7, 4LL << 20, 1LL << 28, (1LL << 28) + 1, LLONG_MAX};
	const int64_t mosts[] = {0, 1, 2, 1000, (1LL << 28) - 1, 1LL << 28, (1LL << 28) + 1, 1LL << 40};
	for (int64_t w : wanted)
		for (int64_t m : mosts) {
			const int64_t c = at::slice_clamp(w, m);
			CHECK(c == ref_clamp(w, m) && c == ref_clamp_local(w, m), "wanted %lld most %lld: %lld", (long long)w, (long long)m, (long long)c);
			CHECK(c >= 1 && c <= (1LL << 28) && c <= std::max<int64_t>(m, 1) && (w < 1 ? c == 1 : c <= w), "wanted %lld most %lld: %lld", (long long)w, (long long)m, (long long)c);
		}
	CHECK(at::slice_clamp(at::kSliceDefault, 0) == 1 && at::slice_clamp(at::kSliceDefault, 1) == 1, "most = 0 and 1");
	CHECK(at::slice_clamp(at::kSliceDefault, 1LL << 28) == 4LL << 20 && at::slice_clamp(1LL << 40, 1LL << 28) == 1LL << 28, "most = 2^28");
	CHECK(at::slice_clamp(0, 100) == 1 && at::slice_clamp(-7, 100) == 1, "a wanted size below 1");
}

/* what the entries' read-backs did with a key, and what the tail of at_scan_hits made of a hit */
static void ref_decode(uint64_t key, int enc, int32_t *rank, int32_t *target, int32_t *strand)
{
	*rank = (int32_t)((uint32_t)(key >> 32) ^ 0x80000000u);
	const uint32_t low = ~(uint32_t)key;
	*target = (int32_t)(low >> enc);
	*strand = enc ? (int32_t)(low & 1u) : 0;
}
static uint64_t ref_encode(int32_t rank, int32_t target, int strand, bool rev)
{
	const uint32_t low = ~(uint32_t)(rev ? ((uint32_t)target << 1) | (uint32_t)strand : (uint32_t)target);
	return ((unsigned long long)((uint32_t)rank ^ 0x80000000u) << 32) | low;
}

static void check_keys()
{
	const int32_t ranks[] = {INT32_MIN + 1, -1000, -1, 0, 1, 77, INT32_MAX};
	for (int enc = 0; enc < 2; ++enc) {
		const int32_t tmost = enc ? (1 << 30) - 1 : INT32_MAX - 1;
		for (int32_t r : ranks)
			for (int32_t t : {0, 1, 12345, tmost})
				for (int st = 0; st <= enc; ++st) {
					const uint64_t key = at::list_key(r, t, st, enc);
					const at::ListKey k = at::list_key_decode(key, enc);
					int32_t rr, rt, rs;
					ref_decode(key, enc, &rr, &rt, &rs);
					CHECK(key != 0 && key == ref_encode(r, t, st, enc != 0), "rank %d target %d strand %d enc %d: key %llx", r, t, st, enc, (unsigned long long)key);
					CHECK(k.rank == r && k.target == t && k.strand == st, "rank %d target %d strand %d enc %d comes back as %d %d %d", r, t, st, enc, k.rank, k.target, k.strand);
					CHECK(k.rank == rr && k.target == rt && k.strand == rs, "decode differs from the entries' read-back");
				}
		/* key order is the ranking: higher rank, then smaller target, then strand 0 */
		for (int n = 0; n < 4000; ++n) {
			const int32_t r1 = n % 3 ? (int32_t)between(-50, 50) : ranks[rnd() % 7], r2 = n % 5 ? (int32_t)between(-50, 50) : ranks[rnd() % 7];
			const int32_t t1 = (int32_t)(n % 7 ? between(0, 9) : between(0, tmost)), t2 = (int32_t)(n % 11 ? between(0, 9) : between(0, tmost));
			const int s1 = enc ? (int)(rnd() & 1) : 0, s2 = enc ? (int)(rnd() & 1) : 0;
			const bool first = r1 != r2 ? r1 > r2 : t1 != t2 ? t1 < t2 : s1 < s2;
			const bool same = r1 == r2 && t1 == t2 && s1 == s2;
			const uint64_t k1 = at::list_key(r1, t1, s1, enc), k2 = at::list_key(r2, t2, s2, enc);
			CHECK(same ? k1 == k2 : first == (k1 > k2), "(%d %d %d) against (%d %d %d), enc %d", r1, t1, s1, r2, t2, s2, enc);
		}
	}
}

static void check_pieces()
{
	for (int n = 0; n < 3000; ++n) {
		const int64_t nh = between(0, 60), hit_cap = between(1, 9), ops_cap = between(1, 400);
		std::vector<int64_t> need((size_t)nh);
		for (auto &x : need) x = rnd() % 9 ? between(0, 120) : between(300, 900);
		std::vector<int> covered((size_t)nh, 0);
		for (int64_t a = 0, b; a < nh; a = b) {
			int64_t ops = -1;
			b = at::piece_end(a, nh, hit_cap, ops_cap, [&](int64_t e) { return need[(size_t)e]; }, &ops);
			/* the entries' loop */
			int64_t rb, rops = 0;
			for (rb = a; rb < nh && rb - a < hit_cap; ++rb) {
				if (rb > a && rops + need[(size_t)rb] > ops_cap) break;
				rops += need[(size_t)rb];
			}
			CHECK(b == rb && ops == rops, "piece from %lld: end %lld ops %lld, expected %lld %lld", (long long)a, (long long)b, (long long)ops, (long long)rb, (long long)rops);
			CHECK(b > a && b <= nh, "empty piece at %lld", (long long)a);
			if (b <= a) return;
			CHECK(b - a <= hit_cap && (ops <= ops_cap || b - a == 1), "piece [%lld, %lld) of %lld op bytes: caps %lld, %lld", (long long)a, (long long)b, (long long)ops, (long long)hit_cap, (long long)ops_cap);
			CHECK(b == nh || b - a == hit_cap || ops + need[(size_t)b] > ops_cap, "piece [%lld, %lld) ends early", (long long)a, (long long)b);
			for (int64_t e = a; e < b; ++e) ++covered[(size_t)e];
			CHECK(b == at::piece_end(a, nh, hit_cap, ops_cap, [&](int64_t e) { return need[(size_t)e]; }), "without the sum");
		}
		for (int64_t e = 0; e < nh; ++e) CHECK(covered[(size_t)e] == 1, "hit %lld in %d pieces", (long long)e, covered[(size_t)e]);
	}
}

static void check_fit()
{
	for (int n = 0; n < 3000; ++n) {
		const int64_t ne = between(0, 40);
		std::vector<int64_t> off((size_t)ne + 1, 0);
		for (int64_t e = 0; e < ne; ++e) off[(size_t)e + 1] = off[(size_t)e] + (rnd() % 4 ? between(1, 30) : 0);
		auto ref = [&](int64_t cap) {
			int64_t fit = 0;
			for (int64_t e = 0; e < ne; ++e) if (off[(size_t)e + 1] <= cap) fit = off[(size_t)e + 1]; else break;
			return fit;
		};
		CHECK(at::prefix_fit(off.data(), ne, 0) == ref(0) && ref(0) == 0, "capacity 0: %lld", (long long)at::prefix_fit(off.data(), ne, 0));
		CHECK(at::prefix_fit(off.data(), ne, -3) == 0, "a negative capacity");
		CHECK(at::prefix_fit(off.data(), ne, off[(size_t)ne]) == off[(size_t)ne] && at::prefix_fit(off.data(), ne, LLONG_MAX) == off[(size_t)ne], "everything fits");
		for (int64_t e = 0; e < ne; ++e) {
			const int64_t end = off[(size_t)e + 1];
			CHECK(at::prefix_fit(off.data(), ne, end) == ref(end) && ref(end) == end, "capacity = the end of entry %lld", (long long)e);
			if (end > off[(size_t)e]) CHECK(at::prefix_fit(off.data(), ne, end - 1) == off[(size_t)e], "one word short of entry %lld", (long long)e);
		}
		const int64_t cap = between(0, off[(size_t)ne] + 5);
		CHECK(at::prefix_fit(off.data(), ne, cap) == ref(cap), "capacity %lld", (long long)cap);
	}
}

/* the per-block loops of the local scan (every target, caller order) and of the fit scan (the block's targets) as they stood */
struct RefTiles { std::vector<long long> tpre[2]; int64_t tiles; int32_t rag_most; };
static RefTiles ref_tiles_local(const std::vector<int32_t> &t_len, int32_t tile, int64_t ov)
{
	const int64_t nt = (int64_t)t_len.size();
	RefTiles r;
	for (auto &v : r.tpre) v.assign((size_t)nt + 1, 0);
	r.rag_most = 0;
	for (int64_t t = 0; t < nt; ++t) {
		const int64_t n = at::localscan_swept(t_len[(size_t)t], tile, ov), nf = at::localscan_swept_full(t_len[(size_t)t], tile, ov);
		const int64_t d = at::localscan_dropped(t_len[(size_t)t], tile, ov);
		r.tpre[0][(size_t)t + 1] = r.tpre[0][(size_t)t] + nf;
		r.tpre[1][(size_t)t + 1] = r.tpre[1][(size_t)t] + (n - nf);
		for (int64_t k2 = nf; k2 < n; ++k2) {
			const int64_t x = at::localscan_swept_tile(k2, d);
			r.rag_most = std::max<int32_t>(r.rag_most, (int32_t)(at::localscan_tile_end(x, tile, ov, t_len[(size_t)t]) - at::localscan_tile_start(x, tile, ov)));
		}
	}
	r.tiles = r.tpre[0][(size_t)nt] + r.tpre[1][(size_t)nt];
	return r;
}
static RefTiles ref_tiles_fit(const std::vector<int32_t> &tls, int64_t ta, int64_t ntb, int32_t l1, int32_t tile, int64_t ov)
{
	RefTiles r;
	r.rag_most = 0;
	for (auto &v : r.tpre) v.assign((size_t)ntb + 1, 0);
	for (int64_t t = 0; t < ntb; ++t) {
		const int32_t l2 = tls[(size_t)(ta + t)];
		const int64_t n = at::fitscan_swept(l1, l2, tile, ov), nf = at::fitscan_swept_full(l1, l2, tile, ov);
		const int64_t d = at::fitscan_dropped(l1, l2, tile, ov);
		r.tpre[0][(size_t)t + 1] = r.tpre[0][(size_t)t] + nf;
		r.tpre[1][(size_t)t + 1] = r.tpre[1][(size_t)t] + (n - nf);
		for (int64_t k2 = nf; k2 < n; ++k2) {
			const int64_t x = at::fitscan_swept_tile(k2, d);
			r.rag_most = std::max<int32_t>(r.rag_most, (int32_t)(at::fitscan_tile_end(x, tile, ov, l2) - at::fitscan_tile_start(x, tile, ov)));
		}
	}
	r.tiles = r.tpre[0][(size_t)ntb] + r.tpre[1][(size_t)ntb];
	return r;
}

static void check_block_tiles()
{
	const int m = 2, u = -2, o = -5, e = -2;
	long long blocks = 0, ragged = 0, full = 0, dropped = 0;
	for (int32_t l1 : {1, 24, 37, 150, 1024})
		for (int32_t T : {16, 64, 1024})
			for (int fit = 0; fit < 2; ++fit)
				for (int use_cutoff = 0; use_cutoff < 2; ++use_cutoff) {
					const int32_t cutoff = m * l1 / 2;
					const int64_t ov = fit ? at::fitscan_overlap(l1, use_cutoff, cutoff, m, u, o, e) : at::localscan_overlap(l1, use_cutoff, cutoff, m, u, o, e);
					/* around every edge: empty, one short of the query, the query, one tile, the full shape and its neighbours, whole tiles, one past */
					std::vector<int32_t> t_len;
					for (int64_t l2 : {(int64_t)0, (int64_t)l1 - 1, (int64_t)l1, (int64_t)T, T + ov - 1, T + ov, T + ov + 1, 5 * (int64_t)T, 5 * (int64_t)T + 1, 3 * (int64_t)T + ov,
					                   3 * (int64_t)T + ov + 1})
						t_len.push_back((int32_t)l2);
					std::vector<long long> tpre[2];
					tpre[0].assign(3, 77);       /* (what an earlier block left is overwritten) */
					auto same = [&](const at::BlockTiles &b, const RefTiles &r, const char *what) {
						CHECK(tpre[0] == r.tpre[0] && tpre[1] == r.tpre[1] && b.tiles == r.tiles && b.rag_most == r.rag_most,
						      "%s: l1=%d tile=%d ov=%lld cutoff=%d: %lld tiles, longest ragged %d; the loop has %lld and %d", what, l1, T, (long long)ov, use_cutoff,
						      (long long)b.tiles, b.rag_most, (long long)r.tiles, r.rag_most);
						++blocks; ragged += r.tpre[1].back() > 0; full += r.tpre[0].back() > 0;
					};
					if (!fit) {
						same(at::block_tiles(t_len.data(), (int64_t)t_len.size(), T, ov, tpre), ref_tiles_local(t_len, T, ov), "local");
						for (int32_t l2 : t_len) dropped += at::localscan_dropped(l2, T, ov) > 0;
						continue;
					}
					/* fit: the targets by length, the block those no shorter than the query (the shorter ones never reach the function) */
					std::vector<int32_t> tls = t_len;
					std::stable_sort(tls.begin(), tls.end());
					const int64_t nt = (int64_t)tls.size(), ta = std::lower_bound(tls.begin(), tls.end(), l1) - tls.begin();
					same(at::block_tiles(tls.data() + ta, nt - ta, T, ov, tpre), ref_tiles_fit(tls, ta, nt - ta, l1, T, ov), "fit block");
					same(at::block_tiles(tls.data(), 0, T, ov, tpre), ref_tiles_fit(tls, 0, 0, l1, T, ov), "no targets");
				}
	/* (the cases do reach the paths they are chosen for) */
	CHECK(blocks == 5 * 3 * (2 + 2 * 2) && ragged > 0 && full > 0 && dropped > 0, "%lld blocks, %lld with ragged tiles, %lld with full ones, %lld targets with dropped tiles", blocks,
	      ragged, full, dropped);
}

int main()
{
	for (int strands = 1; strands <= 3; ++strands) {
		for (int64_t nq : {0, 1, 2, 3, 200}) for (int nl : {1, 2}) check_order(nq, strands, nl);
		for (int n = 0; n < 1200; ++n) check_order(between(0, 200), strands, (int)between(1, 5));
	}
	check_clamp();
	check_keys();
	check_pieces();
	check_fit();
	check_block_tiles();
	if (g_failures) { printf("queryplan_check: %d failures\n", g_failures); return 1; }
	printf("queryplan_check: ok\n");
	return 0;
}
