/*
 * aligntools_hip.h -- C ABI of the MI355X (gfx950) alignment shim.
 *
 * This is the drop-in boundary for the dynamic-programming hot path of
 * r3fang/alignTools: the O(l1*l2) matrix fill + pointer traceback of
 *
 *     align_gla               reference src/alignment.h:417-473 (+ :372-412)
 *     align_local_affine      reference src/alignment.h:805-847 (+ :766-800)
 *     align_fit_affine_jump   reference src/alignment.h:596-694 (+ :558-592)
 *     align_overlap           reference src/alignment.h:926-964 (+ :896-922)
 *     edit_dist               reference src/alignment.h:291-315
 *
 * The reference has no FFI of its own (it is one C translation unit); these
 * entry points are what its five main_* drivers (alignment.h:318,476,698,851,
 * 967) call instead of the align_*() functions -- see include/aligntools.h for
 * the reference-shaped single-pair wrappers and INTEGRATION.md for the patch.
 *
 * Plain C: pointers and sizes only, int return (0 = AT_OK, negative = error,
 * text via at_last_error), caller-owned buffers, one handle per thread.
 * There is NO CPU fallback: without a HIP device at_init fails.
 */
#ifndef ALIGNTOOLS_HIP_H
#define ALIGNTOOLS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* sub-commands (reference src/main.c:39-43) */
enum { AT_MODE_GLOBAL = 0, AT_MODE_LOCAL = 1, AT_MODE_FIT = 2, AT_MODE_OVERLAP = 3, AT_MODE_EDIT = 4 };

/* traceback ops, emitted END -> START (the order the reference's trace_back_*
 * loops produce characters before strrev, alignment.h:372-412) */
enum { AT_OP_MID = 0,   /* (s1[i-1], s2[j-1]); i--, j--                    */
       AT_OP_LOW = 1,   /* (s1[i-1], '-');     i--                          */
       AT_OP_UPP = 2,   /* ('-', s2[j-1]);     j--                          */
       AT_OP_JUMP = 3   /* ('-', s2[j-1]);     j--   fit jump state         */ };

/* state the traceback starts in (reference LOW/MID/UPP, alignment.h:31-33) */
enum { AT_ST_LOW = 1, AT_ST_MID = 2, AT_ST_UPP = 3 };

enum { AT_OK = 0,
       AT_ERR_ARG = -1,        /* NULL / negative size / unknown mode                  */
       AT_ERR_NODEVICE = -2,   /* no HIP device / HIP runtime error                    */
       AT_ERR_RANGE = -3,      /* |score| could leave the exact int32 range            */
       AT_ERR_DOMAIN = -4,     /* input outside the domain the reference defines       */
       AT_ERR_FIT_ORDER = -5,  /* fit: first sequence longer than the second (:599)    */
       AT_ERR_NOMEM = -6 };

typedef struct at_handle at_handle;

/* Bind to one GPU.  One process (or thread) per GPU: n_devices must be 1.
 * device_ids == NULL selects the current device. */
int at_init(const int *device_ids, int n_devices, at_handle **out);
void at_destroy(at_handle *h);
/* Text of the last error on handle h; h == NULL: of the calling thread's last failure without a handle (at_init). */
const char *at_last_error(const at_handle *h);

/* Scoring block = the reference's opt_t (alignment.h:57-65, defaults :102-114:
 * o=-5 e=-1 m=1 u=-2 j=-10 s=false).  `sites` are 0-based positions on s2 as
 * parsed from the 2nd record's FASTA comment (alignment.h:243-256); only used
 * by AT_MODE_FIT with use_jump.  The reference's inverted junction predicate
 * (alignment.h:659) is reproduced: M->J may open at column j
 * iff (j-1) is NOT listed. */
int at_set_scoring(at_handle *h, int m, int u, int o, int e, int j,
                   int use_jump, const int *sites, int nsites);

/*
 * Align a batch of independent pairs held in HOST memory.
 *   seq_blob          raw sequence bytes (any alphabet; compared by byte
 *                     equality like alignment.h:449).  All-ACGT batches are packed
 *                     2 bits per base, others 8 bits, both on the GPU.
 *   off1/len1, off2/len2   per pair: byte offset and length of s1 and s2
 *   want_traceback    0 = scores and end cells only
 *   out_score[n]      reference return value (align_*: the double, always an
 *                     integer; edit: the distance)
 *   out_end_i/j[n]    cell the traceback starts from (1-based DP coordinates)
 *   out_state[n]      AT_ST_* start state
 *   out_ops, ops_off[n], out_nops[n]
 *                     ops of pair k are written to out_ops[ops_off[k] ..] (at
 *                     most len1+len2 of them), count in out_nops[k].  Exactly
 *                     out_nops[k] bytes of a slot are written; bytes between and
 *                     behind the slots are never touched, and the slots may come
 *                     in any order (they must not overlap).
 * Any out_* may be NULL if not wanted (out_ops/ops_off/out_nops together).
 */
int at_align_batch(at_handle *h, int mode, int64_t npairs,
                   const uint8_t *seq_blob,
                   const int64_t *off1, const int32_t *len1,
                   const int64_t *off2, const int32_t *len2,
                   int want_traceback,
                   int32_t *out_score, int32_t *out_end_i, int32_t *out_end_j, int32_t *out_state,
                   uint8_t *out_ops, const int64_t *ops_off, int32_t *out_nops);

/*
 * Same, with every buffer already resident in DEVICE memory (HBM) and the
 * sequences already packed (at_pack_batch): the entry the batch driver and
 * bench.py use.  Asynchronous on `stream` (a hipStream_t, NULL = default).
 * A handle owns one work counter, one workspace and one flag word: use it with
 * ONE stream at a time (calls queued on the same stream may follow each other
 * without waiting; a call on another stream needs the earlier ones finished --
 * or its own handle, which is how bench.py keeps three launches in flight).
 * One kind of call makes the host wait although the entry is asynchronous: the first call of a larger shape on a handle.  Its
 * workspace, checkpoint buffer, scan scratch or site mask (a longer second sequence under fit -s) is then freed and allocated
 * anew, and hipFree waits for the device -- which is also what keeps a launch that is still queued from losing its buffer.  A
 * caller who needs launches in flight warms the handle with its largest shapes first, as bench.py does.  at_set_scoring between
 * two queued launches does not wait: the next fit -s launch sends the new site mask up behind the launches before it
 * (tests/test_streams_in_flight.py).
 *   d_seq      packed words; bits = 2 (A,C,G,T -> 0..3, 16 bases per int32,
 *              base k of a sequence in bits [2k%32, 2k%32+1] of word k/16) or
 *              bits = 8 (4 bytes per int32, little endian)
 *   d_woff1/2  per pair WORD offset of s1 / s2 in d_seq
 *   max_len1/2 upper bounds of len1/len2 over the batch (sizes LDS / workspace); a pair
 *              longer than its bound is refused (score INT32_MIN, nops -1), not swept
 *   uniform_shape  non-zero = the caller guarantees len1[k] == max_len1 and
 *              len2[k] == max_len2 for every pair (fixed-length read batches);
 *              enables the packed two-pairs-per-wavefront kernel when the
 *              scores provably fit 16 bits.  0 is always safe: batches of 4096
 *              pairs or more are then checked on the device, and the packed or
 *              the int32 kernel runs accordingly (3 % slower than with the
 *              promise, not 2.5 times).  A pair that breaks
 *              the promise is not swept: it and the pairs sharing its work item
 *              (at most 16; 32 for reads of up to 76 bases) come back with
 *              score INT32_MIN and nops -1.
 */
int at_align_batch_device(at_handle *h, int mode, int64_t npairs,
                          const uint32_t *d_seq, int bits,
                          const int64_t *d_woff1, const int32_t *d_len1,
                          const int64_t *d_woff2, const int32_t *d_len2,
                          int32_t max_len1, int32_t max_len2, int uniform_shape,
                          int want_traceback,
                          int32_t *d_score, int32_t *d_end_i, int32_t *d_end_j, int32_t *d_state,
                          uint8_t *d_ops, const int64_t *d_ops_off, int32_t *d_nops,
                          void *stream);

/*
 * All-vs-all over one read set (BASELINE config "overlap, all-vs-all 50k x 1 kbp reads"): d_woff/d_len
 * describe `nreads` packed reads; work item p in [0, npairs) is the ordered pair (a < b) whose row-major
 * index in the strict upper triangle is first_pair + p, aligned as s1 = read a, s2 = read b.  No per-pair
 * descriptors exist (1.25e9 pairs would need 30 GB of them); outputs are indexed by p.  Ranks of a
 * multi-GPU job take disjoint [first_pair, first_pair + npairs) ranges.
 */
int at_align_allpairs_device(at_handle *h, int mode, int64_t nreads,
                             const uint32_t *d_seq, int bits,
                             const int64_t *d_woff, const int32_t *d_len, int32_t max_len,
                             int64_t first_pair, int64_t npairs, int want_traceback,
                             int32_t *d_score, int32_t *d_end_i, int32_t *d_end_j, int32_t *d_state,
                             uint8_t *d_ops, const int64_t *d_ops_off, int32_t *d_nops,
                             void *stream);

/*
 * All-vs-all with the read set in HOST memory (what `alignTools batch <cmd> --all-vs-all reads.fa` calls): the reads
 * (off[k], len[k] in seq_blob) go up and are packed once; pair p of [first_pair, first_pair + npairs) is aligned as
 * s1 = read a, s2 = read b with (a, b) as in at_align_allpairs_device; outputs are indexed by p - first_pair; pair p's
 * ops go to out_ops[ops_off[p - first_pair] ..] (a slot of len[a] + len[b] bytes).  Not for AT_MODE_FIT (l1 <= l2 is a
 * property of ordered pairs).
 */
int at_align_allpairs(at_handle *h, int mode, int64_t nreads,
                      const uint8_t *seq_blob, const int64_t *off, const int32_t *len,
                      int64_t first_pair, int64_t npairs, int want_traceback,
                      int32_t *out_score, int32_t *out_end_i, int32_t *out_end_j, int32_t *out_state,
                      uint8_t *out_ops, const int64_t *ops_off, int32_t *out_nops);

/*
 * A score threshold for all-vs-all overlap SCORES (at_align_allpairs_device / at_align_allpairs / at_align_allpairs_stream with
 * AT_MODE_OVERLAP and no tracebacks; reads of up to 1 024 bases, ACGT): with enabled != 0 a pair whose score -- the value of
 * align_overlap, alignment.h:926-964 -- is PROVEN to lie below min_score is not swept: its state is 0, its score an upper bound
 * (< min_score) and its end_j 0.  Every other pair (state 2) carries the exact results as without the threshold, whether its score
 * reaches min_score or not.  The proof is an upper bound from the bit-parallel edit distance of the pair with a free start in s1
 * (csrc/at_myers.hip.h): 2 score <= 2 m b - (2 c - m) D'(l1, b), c = min(m - u, m / 2 - o); it needs m >= 0 and 2 c > m (the default
 * scoring of `alignTools overlap`, m = 1 u = -2 o = -5, gives 2 b - 5 D'), otherwise every pair is swept.  enabled = 0 (the default)
 * sweeps every pair.
 */
int at_set_min_score(at_handle *h, int enabled, int32_t min_score);

/*
 * Edit ALIGNMENTS: the alignment behind the number AT_MODE_EDIT returns.  A per-handle setting; enabled = 0 (the default) changes
 * nothing anywhere.  The reference's edit_dist (alignment.h:291-315) has no traceback, so the rule is this library's.  D is its table
 * with the unit mismatch cost: D(i,0) = i, D(0,j) = j, D(i,j) = min(D(i,j-1) + 1, D(i-1,j-1) + (s1[i-1] != s2[j-1]), D(i-1,j) + 1).
 * The op list runs END -> START like every other mode's, from (l1, l2) to (0, 0); at cell (i, j) the first rule that holds:
 *   1. i > 0 && j > 0 && D(i-1,j-1) + (s1[i-1] != s2[j-1]) == D(i,j)    AT_OP_MID, i--, j--
 *   2. i > 0 && D(i-1,j) + 1 == D(i,j)                                  AT_OP_LOW, i--
 *   3. otherwise                                                        AT_OP_UPP, j--
 * score = D(l1,l2), end cell (l1, l2), state AT_ST_MID (what the number-only path returns), nops <= l1 + l2; the number of mismatch
 * columns plus gap columns equals the score.
 * With the setting on
 *   - at_align_batch and at_align_batch_device with AT_MODE_EDIT and want_traceback != 0 deliver the ops in the usual slots (exactly
 *     nops bytes written, nothing else touched); with want_traceback == 0 they take the number-only route as before;
 *   - at_align_batch_strings and at_align_batch_cigar accept AT_MODE_EDIT and run the rendering / CIGAR kernels over those ops.
 * The domain: mismatch cost u == 1, a 2-bit (pure ACGT) batch, max_len1 <= 1 024, and max_len2 no longer than 64 windows of packed
 * words hold in 60 KB of LDS (3 792 bases).  Outside it the call fails with AT_ERR_DOMAIN and a text that names the broken bound;
 * there is no silent fall back to the number alone.  The fill keeps two words per 32 rows and column in the handle's workspace
 * (max_len2 * W * 512 bytes per wavefront of 64 pairs, W = 2 .. 32 words for reads of up to 64 .. 1 024 bases), bounded like the
 * pointer slots of the sweeps; a work item above that bound is AT_ERR_NOMEM.
 * Edit stays number-only, whatever the setting, in the all-pairs entries and in the searches, for 8-bit alphabets, reads beyond
 * 1 024 bases, u != 1, multi-GPU batches and the reference-named single-pair surface of aligntools.h.
 */
int at_set_edit_traceback(at_handle *h, int enabled);

/*
 * Edit INFIX mode: the best match of s1 (a read) inside s2 (a target) -- approximate matching in Myers' sense: the read may start
 * anywhere in the target and end anywhere.  A per-handle setting; enabled = 0 (the default) changes nothing anywhere.  With it on,
 * AT_MODE_EDIT means (the rule is this library's; the reference's edit_dist, alignment.h:291-315, is global only):
 *   table   D(0,j) = 0, D(i,0) = i, D(i,j) = min(D(i,j-1) + 1, D(i-1,j-1) + (s1[i-1] != s2[j-1]), D(i-1,j) + 1)
 *   result  score = min over 0 <= j <= l2 of D(l1,j); end cell (l1, j*) with j* the SMALLEST j that attains the minimum (first wins,
 *           like the local arg-max); state AT_ST_MID.  l1 = 0: score 0, j* = 0.  l2 = 0: score l1, j* = 0.  l1 > l2 is allowed (the
 *           score is then at least l1 - l2)
 *   ops     delivered when at_set_edit_traceback is on as well and want_traceback is set; END -> START from (l1, j*) until i == 0,
 *           at cell (i, j) the first rule that holds:
 *             1. j > 0 && D(i-1,j-1) + (s1[i-1] != s2[j-1]) == D(i,j)    AT_OP_MID, i--, j--
 *             2. D(i-1,j) + 1 == D(i,j)                                  AT_OP_LOW, i--
 *             3. otherwise                                               AT_OP_UPP, j--
 *           (at j == 0 rule 2 always holds.)  The walk ends in (0, j0); nops <= l1 + l2; mismatch columns plus gap columns equal the
 *           score.  j0 is the target start: AT_CG_START_J of the statistics row and the target start column of a PAF line, both
 *           derived as ever from the end cell minus the columns consumed.
 * Examples: ACGT in ACGTACGTACGT: score 0, j* = 4, four MID.  ACGTA in CG: score 3, j* = 2, ops LOW LOW MID MID LOW.
 * at_align_batch, at_align_batch_device, at_align_batch_strings, at_align_batch_cigar, at_search and at_search_strands follow the
 * setting (a search then ranks targets by where the read fits, every (query, target) pair a candidate whatever the lengths; a hit's
 * score, end cell and state are exactly what at_align_batch returns for that pair).
 * The domain is that of the edit alignments: mismatch cost u == 1, a 2-bit (pure ACGT) batch, max_len1 <= 1 024, max_len2 <= 3 792 (64
 * windows of packed words in 60 KB of LDS).  Outside it the call fails with AT_ERR_DOMAIN and a text that names the broken bound; it
 * never falls back to the global number, which under this setting would be a wrong answer.  For the same reason the all-pairs
 * entries in edit mode fail with AT_ERR_DOMAIN while the setting is on, and so does an edit batch on a handle that has joined a
 * multi-process job (at_comm_init: the setting is not broadcast to the other ranks).  The reference-named single-pair surface of aligntools.h never turns it on.
 * Kernels: csrc/at_infix.hip.h; at_last_config begins "myers-infix" (number only) or "myers-infix-tb" (with ops).
 */
int at_set_edit_infix(at_handle *h, int enabled);

/*
 * The same sweep with bounded memory, for triangles too large to hold (C5: 50 000 reads = 1.25e9 pairs = 20 GB of
 * results): scores and end cells only, the triangle cut into slices of at most chunk_pairs pairs (<= 0: 4 Mi); `fn`
 * is called once per slice, in pair order, on the calling thread, while the GPU already sweeps the next slice.  The
 * arrays it sees (indexed by pair - first) are valid during the call only; a non-zero return stops the sweep
 * (AT_ERR_ARG).  at_align_allpairs without tracebacks is this entry with a callback that copies into its out arrays.
 */
typedef int (*at_allpairs_chunk_fn)(void *user, int64_t first, int64_t npairs,
                                    const int32_t *score, const int32_t *end_i, const int32_t *end_j, const int32_t *state);
int at_align_allpairs_stream(at_handle *h, int mode, int64_t nreads,
                             const uint8_t *seq_blob, const int64_t *off, const int32_t *len,
                             int64_t first_pair, int64_t npairs, int64_t chunk_pairs,
                             at_allpairs_chunk_fn fn, void *user);

/*
 * Every query against every target: for each query q the best k hits (1 <= k <= 64) in rank order.
 *   queries q_off/q_len in q_blob, targets t_off/t_len in t_blob (host memory, any alphabet, like at_align_batch)
 *   rank: the four affine modes: higher score first; AT_MODE_EDIT: smaller distance first; ties: smaller target index first
 *   use_cutoff != 0: only hits that rank at least as well as `cutoff` (score >= cutoff; edit: distance <= cutoff)
 *   out_* hold nq*k entries, row q = hits of query q; out_nhits[q] <= k; unused entries have target -1
 *   score / end_i / end_j / state of a hit are exactly what at_align_batch returns for that (query, target) pair
 *   AT_MODE_FIT: a pair whose query is longer than its target is not a candidate (no error); with use_jump the
 *   handle's site list applies to every target, as in a pair-list batch
 * Synchronous; no tracebacks (pass the hit pairs to at_align_batch / at_align_batch_strings for those).  Queries and targets go up
 * as one read set; only the nq*k list entries come back.  at_set_min_score does not apply to a search.  nq == 0 writes nothing;
 * nt == 0 gives every query 0 hits.  at_last_config: "search: B blocks, S slices, k=K; " and the first slice's sweep.
 */
int at_search(at_handle *h, int mode,
              int64_t nq, const uint8_t *q_blob, const int64_t *q_off, const int32_t *q_len,
              int64_t nt, const uint8_t *t_blob, const int64_t *t_off, const int32_t *t_len,
              int k, int use_cutoff, int32_t cutoff,
              int32_t *out_target, int32_t *out_score, int32_t *out_end_i, int32_t *out_end_j,
              int32_t *out_state, int32_t *out_nhits);

/*
 * Reverse complement.  The complement of a byte is stated once, here, as (from, to) pairs of upper-case letters -- the IUPAC
 * nucleotide codes, U read as T -- and holds for the lower-case letters likewise; S, W, N and every other byte value map to
 * themselves.  The host helper and the device kernel (csrc/at_revcomp.hip) build their 256-entry table from this string.
 */
#define AT_COMPLEMENT_PAIRS "ATTACGGCUARYYRKMMKBVVBDHHD"
/* Host helper: out[0..len) = the reverse complement of s[0..len) under the table above; out may not alias s. */
int at_revcomp(const uint8_t *s, int32_t len, uint8_t *out);
/*
 * The same for `nseq` PACKED reads already in device memory (the word layout of at_align_batch_device, bits = 2 or 8): for r in
 * [0, nseq) the words of the reverse complement of the read at d_seq + d_woff[r] (d_len[r] bases) are written to
 * d_out + d_out_woff[r]; d_out_woff == NULL: the same offsets as d_woff.  Bit for bit what at_pack_batch gives for the
 * reverse-complemented bytes: ceil(len / bases per word) words and the zero slack word behind them, zero bits behind the last
 * base; no other word of d_out is written.  d_out must not overlap d_seq.  Asynchronous on `stream`; the same handle / stream
 * rules as at_align_batch_device.
 */
int at_revcomp_device(at_handle *h, int64_t nseq, const uint32_t *d_seq, int bits,
                      const int64_t *d_woff, const int32_t *d_len,
                      uint32_t *d_out, const int64_t *d_out_woff, void *stream);

/*
 * at_search on one or both strands of the queries.  strands = AT_STRAND_FWD: at_search itself (out_strand may be NULL);
 * AT_STRAND_REV: every query is searched as its reverse complement; AT_STRAND_BOTH: as given and as its reverse complement.
 *   a hit is (target, strand): out_strand[e] is 0 for the query as given, 1 for its reverse complement, -1 for an unused entry
 *   score / end_i / end_j / state of a strand-1 hit are exactly what at_align_batch returns for the pair (reverse complement of
 *   the query under at_revcomp, target): end_i counts along the reverse-complemented query.  Targets are never complemented,
 *   so a fit -s site list keeps its meaning
 *   rank: better score first, ties to the smaller target index, then strand 0 before strand 1; a query equal to its own
 *   reverse complement yields two hits per target, adjacent in its list
 * The queries go up once, as given; the reverse strand is made on the device from the packed words (at_revcomp_device's
 * kernel).  With a reverse strand the call needs nt < 2^30 and 2 nq + nt < 2^31 (AT_ERR_ARG beyond).  at_last_config reads
 * "search: B blocks, S slices, k=K, strands=rev; " or "... k=K, strands=both; " and the first slice's sweep.
 */
enum { AT_STRAND_FWD = 1, AT_STRAND_REV = 2, AT_STRAND_BOTH = 3 };
int at_search_strands(at_handle *h, int mode,
                      int64_t nq, const uint8_t *q_blob, const int64_t *q_off, const int32_t *q_len,
                      int64_t nt, const uint8_t *t_blob, const int64_t *t_off, const int32_t *t_len,
                      int k, int use_cutoff, int32_t cutoff, int strands,
                      int32_t *out_target, int32_t *out_score, int32_t *out_end_i, int32_t *out_end_j,
                      int32_t *out_state, int32_t *out_strand, int32_t *out_nhits);

/*
 * Output rendering on the GPU: what trace_back_* + strrev produce (alignment.h:372-412,
 * 558-592, 766-800, 896-922, 172-184) -- the two gapped strings, in reading order -- from the op codes and end
 * cells at_align_batch_device left in HBM and the same packed sequences.  Pair k's strings are written to
 * d_r1/d_r2 at byte offset d_str_off[k] (NULL = d_ops_off[k]), d_nops[k] characters each, followed by a 0 byte
 * when nul_terminate (the slot then needs len1+len2+1 bytes).  Asynchronous on `stream`.
 */
int at_render_batch_device(at_handle *h, int64_t npairs,
                           const uint32_t *d_seq, int bits,
                           const int64_t *d_woff1, const int64_t *d_woff2,
                           const int32_t *d_end_i, const int32_t *d_end_j,
                           const uint8_t *d_ops, const int64_t *d_ops_off, const int32_t *d_nops,
                           uint8_t *d_r1, uint8_t *d_r2, const int64_t *d_str_off, int nul_terminate,
                           void *stream);

/*
 * CIGAR compaction for the result gather (sizes first, then one payload).  Writes the exclusive
 * prefix sums of d_nops to d_packed_off[0 .. npairs] (d_packed_off[npairs] = total bytes) and copies pair k's ops
 * from its slot to d_packed[d_packed_off[k] ..).  Pairs that would end beyond packed_cap are not copied: compare the
 * total with the capacity.  Asynchronous on `stream`.
 */
int at_compact_ops_device(at_handle *h, int64_t npairs,
                          const uint8_t *d_ops, const int64_t *d_ops_off, const int32_t *d_nops,
                          uint8_t *d_packed, int64_t packed_cap, int64_t *d_packed_off, void *stream);

/*
 * at_align_batch with the rendering done on the GPU: instead of op codes the caller receives the reference's
 * two strings per pair (0-terminated) at out_r1/out_r2 + str_off[k], slots of len1[k]+len2[k]+1 bytes, and
 * their common length in out_len[k].  AT_MODE_EDIT only with at_set_edit_traceback on (edit_dist returns a number only).
 */
int at_align_batch_strings(at_handle *h, int mode, int64_t npairs,
                           const uint8_t *seq_blob,
                           const int64_t *off1, const int32_t *len1,
                           const int64_t *off2, const int32_t *len2,
                           int32_t *out_score, int32_t *out_end_i, int32_t *out_end_j, int32_t *out_state,
                           char *out_r1, char *out_r2, const int64_t *str_off, int32_t *out_len);

/*
 * Run-length CIGARs and alignment statistics: what a mapper's users consume, made from the op codes, the end cell
 * and the two sequences.  A column's class is a BAM op code of "MIDNSHP=X": AT_OP_MID with equal bytes '=' (7), with unequal bytes
 * 'X' (8), AT_OP_LOW 'I' (1), AT_OP_UPP 'D' (2), AT_OP_JUMP 'N' (3, the spliced gap of fit -s); with AT_CIGAR_M in `flags`, '=' and
 * 'X' are both 'M' (0) and merge into one run.  A word is (run length << 4) | code; words are in reading order (START -> END, the
 * order of the rendered strings).  stats[8]: AT_CG_START_I / AT_CG_START_J (the end cell minus the rows / columns consumed: 0-based,
 * inclusive), equal columns, unequal columns (both filled with either flavour), I bases, D bases, N bases, I runs + D runs.
 * An op code above 3 or a walk below row / column 0 is an inconsistent list: ncigar = -1, a statistics row of -1, no word written.
 */
enum { AT_CIGAR_M = 1 };
enum { AT_CG_START_I = 0, AT_CG_START_J = 1, AT_CG_EQUAL = 2, AT_CG_UNEQUAL = 3, AT_CG_INS = 4, AT_CG_DEL = 5, AT_CG_SKIP = 6,
       AT_CG_GAPS = 7 };

/* Host helper, the sibling of at_render: ops (END -> START) + end cell -> CIGAR words and statistics.  cigar may be NULL (counts and
 * statistics only), else it needs nops words.  AT_ERR_DOMAIN for an inconsistent list (*ncigar = -1, stats all -1), AT_ERR_ARG for
 * NULL / negative arguments.  No handle, no GPU. */
int at_cigar(const uint8_t *ops, int32_t nops,
             const uint8_t *s1, int32_t end_i, const uint8_t *s2, int32_t end_j, int flags,
             uint32_t *cigar, int32_t *ncigar, int32_t stats[8]);

/*
 * The same on the GPU, from what at_align_batch_device left in HBM (arguments as at_render_batch_device): d_ncigar[k] runs and
 * d_stats[k][8] (may be NULL) per pair, the exclusive prefix sums of the run counts in d_cigar_off[0 .. npairs]
 * (d_cigar_off[npairs] = total words), pair k's words at d_cigar[d_cigar_off[k] ..).  Pairs that would end beyond cigar_cap are not
 * written and no other word of d_cigar is touched: compare the total with the capacity.  A pair with d_nops[k] < 0 or an
 * inconsistent list gets d_ncigar[k] = -1 and a statistics row of -1 and counts as 0 words.  npairs == 0 writes d_cigar_off[0] = 0
 * only.  Asynchronous on `stream`.
 */
int at_cigar_batch_device(at_handle *h, int64_t npairs,
                          const uint32_t *d_seq, int bits,
                          const int64_t *d_woff1, const int64_t *d_woff2,
                          const int32_t *d_end_i, const int32_t *d_end_j,
                          const uint8_t *d_ops, const int64_t *d_ops_off, const int32_t *d_nops,
                          int flags, int32_t *d_ncigar, int32_t *d_stats, int64_t *d_cigar_off,
                          uint32_t *d_cigar, int64_t cigar_cap, void *stream);

/*
 * at_align_batch with CIGARs made on the GPU: neither op codes nor strings cross the link, only the fixed-size results, the
 * statistics rows (out_stats[k][8]) and the packed words.  out_ncigar[k] runs per pair, out_cigar_off[0 .. npairs] their exclusive
 * prefix sums in pair order (out_cigar_off[npairs] = total words): both always complete.  out_cigar receives the words of the pairs
 * that end within cigar_cap; a caller whose buffer was too small compares the total with it and calls again.  AT_MODE_EDIT only with at_set_edit_traceback on.
 */
int at_align_batch_cigar(at_handle *h, int mode, int64_t npairs,
                         const uint8_t *seq_blob,
                         const int64_t *off1, const int32_t *len1,
                         const int64_t *off2, const int32_t *len2,
                         int flags,
                         int32_t *out_score, int32_t *out_end_i, int32_t *out_end_j, int32_t *out_state,
                         int32_t *out_stats, int32_t *out_ncigar, int64_t *out_cigar_off,
                         uint32_t *out_cigar, int64_t cigar_cap);

/*
 * Reads against LONG targets: what at_search_strands delivers under at_set_edit_infix -- for each query the best
 * k hits (1 <= k <= 64) over the targets, a hit being the best match of the query (or of its reverse complement) INSIDE a target:
 * D(0,j) = 0, D(i,0) = i, score = min over j of D(l1,j), end cell (l1, j*) with the smallest such j, state AT_ST_MID -- with no
 * bound on the target length (any int32).  A target is cut into overlapping tiles that are swept independently; the minimum over
 * the tiles is exact for every pair that scores <= the query length (with use_cutoff: <= min(query length, cutoff); the other
 * pairs are no hits anyway).  Queries of up to 1 024 bases, pure ACGT, u == 1; one GPU.
 *   rank: smaller distance first, then the smaller target index, then strand 0 before strand 1
 *   out_target .. out_nhits as in at_search_strands (nq*k entries, unused entries -1; out_strand may be NULL for AT_STRAND_FWD);
 *   end_j is the ABSOLUTE column j* of the target
 *   tile_cols: the columns a lane owns, a multiple of 16; 0 = the library's default (2 048).  The results do not depend on it
 *   the four CIGAR outputs are either all NULL or laid out as in at_align_batch_cigar over the nq*k entries (out_cigar_off has
 *   nq*k + 1 entries; an unused entry has 0 runs and a statistics row of -1; flags: AT_CIGAR_M or 0).  The ops of a hit are those of
 *   the three-way rule above on the full table; AT_CG_START_J is absolute.  They are made in a window of the target around the hit
 *   (at most 2 * 1 024 + 15 columns), and a window that does not reproduce its hit is AT_ERR_RANGE, never a silent result
 * The handle's at_set_edit_infix / at_set_edit_traceback settings neither matter nor change.  Synchronous.  nq == 0 writes
 * nothing; nt == 0 gives every query 0 hits.  AT_ERR_DOMAIN: u != 1, a byte outside ACGT, a query longer than 1 024, a handle of a
 * multi-process job; AT_ERR_ARG: k outside 1..64, strands outside 1..3, tile_cols negative or no multiple of 16.
 * at_last_config: "scan: tile=T overlap<=OV groups=G k=K strands=fwd|rev|both, B blocks, S slices; myers-scan bits=2 words/lane=W ..."
 * and, with CIGARs, "; windows: " and the window pass's text.
 */
int at_scan(at_handle *h,
            int64_t nq, const uint8_t *q_blob, const int64_t *q_off, const int32_t *q_len,
            int64_t nt, const uint8_t *t_blob, const int64_t *t_off, const int32_t *t_len,
            int k, int use_cutoff, int32_t cutoff, int strands, int32_t tile_cols, int flags,
            int32_t *out_target, int32_t *out_score, int32_t *out_end_i, int32_t *out_end_j,
            int32_t *out_state, int32_t *out_strand, int32_t *out_nhits,
            int32_t *out_stats, int32_t *out_ncigar, int64_t *out_cigar_off,
            uint32_t *out_cigar, int64_t cigar_cap);
/* Host helper (no handle, no GPU): how at_scan cuts a pair of len1 x len2 -- *tile = the columns a lane owns (tile_cols, or the
 * default for 0), *overlap = the warm-up columns in front of a tile, round16up(len1 + c) with c = len1 without a cutoff and
 * min(len1, cutoff) with one, *ngroups = ceil(len2 / (64 * tile)), at least 1.  Any out pointer may be NULL.  AT_ERR_ARG for a
 * negative length and for a tile_cols that is negative or no multiple of 16. */
int at_scan_plan(int32_t len1, int32_t len2, int use_cutoff, int32_t cutoff, int32_t tile_cols,
                 int32_t *tile, int32_t *overlap, int64_t *ngroups);

/*
 * Smith-Waterman of reads against LONG targets: what at_search_strands(AT_MODE_LOCAL) delivers -- for each query
 * the best k hits (1 <= k <= 64) over the targets, one per (query, strand, target), a hit being exactly what
 * at_align_batch(AT_MODE_LOCAL) returns for (query or its reverse complement, target): the score, the end cell (i*, j*) = the first
 * maximum of M in row-major order, state AT_ST_MID -- with no bound on the target length (any int32).  A target is cut into
 * overlapping tiles that are swept as ordinary local pairs by the batch kernels; the best over the tiles is exact for every pair
 * that scores >= max(1, cutoff) (the other pairs are no hits under the cutoff anyway; without one every pair is exact).
 *   domain: the handle's scoring with m >= 1, o <= -1, e <= -1 (u anything); queries of 1 .. 1 024 bases with max(m, u) * length
 *   < 2^20; targets of 1 .. 2^31 - 1 bases; any alphabet at_search takes; one GPU
 *   rank: higher score first, then the smaller target index, then strand 0 before strand 1 (at_search_strands' order)
 *   out_target .. out_nhits as in at_search_strands; end_j is the ABSOLUTE column j* of the target
 *   tile_cols: the columns a tile owns, a multiple of 16; 0 = the library's default (1 024).  The results do not depend on it
 *   the four CIGAR outputs are either all NULL or laid out as in at_scan (an unused entry: 0 runs, a row of -1, no room).  The ops of a hit are those of the reference's walk on the
 *   full table; AT_CG_START_J is absolute.  They are made in a window of the target that ends in j*, and a window that does not
 *   reproduce its hit is AT_ERR_RANGE, never a silent result
 * at_set_min_score neither matters nor changes.  Synchronous.  nq == 0 writes nothing; nt == 0 gives every query 0 hits.
 * AT_ERR_DOMAIN: the scoring, an empty or too long query, an empty target, a handle of a multi-process job; AT_ERR_ARG: k outside
 * 1..64, strands outside 1..3, tile_cols negative or no multiple of 16.  AT_ERR_RANGE, before anything is swept: a tile is a pair of
 * the batch entry and has its exact-score bound, max(|m|,|u|,|o|,|e|,|j|) * (l1 + T + ov + 2) < 2^24 with ov = round16up(l1 +
 * floor((max(m,u) * l1 - c) / min(|o|,|e|))) -- large scores with cheap gaps (m = 200, o = e = -1 at 1 024 bases) are outside it.
 * at_last_config: "local-scan: tile=T overlap<=OV tiles=N k=K strands=fwd|rev|both, B blocks, S slices; " + the first slice's sweep
 * text + " sweep=..ms" (the device time of the sweep phase, as at_scan reports it) and, with CIGARs, "; windows: " and the window
 * pass's text.
 */
int at_scan_local(at_handle *h,
                  int64_t nq, const uint8_t *q_blob, const int64_t *q_off, const int32_t *q_len,
                  int64_t nt, const uint8_t *t_blob, const int64_t *t_off, const int32_t *t_len,
                  int k, int use_cutoff, int32_t cutoff, int strands, int32_t tile_cols, int flags,
                  int32_t *out_target, int32_t *out_score, int32_t *out_end_i, int32_t *out_end_j,
                  int32_t *out_state, int32_t *out_strand, int32_t *out_nhits,
                  int32_t *out_stats, int32_t *out_ncigar, int64_t *out_cigar_off,
                  uint32_t *out_cigar, int64_t cigar_cap);
/* Host helper (no handle, no GPU): how at_scan_local cuts a pair of len1 x len2 under the scoring m / u / o / e -- *tile = the columns
 * a tile owns, *overlap = ov = round16up(len1 + g(len1, c)), the columns in front of them, *ntiles = ceil(len2 / tile), *nfull = the
 * leading tiles of the full shape len1 x (tile + ov).  Tile n sweeps the columns (max(0, n tile - ov), min(len2, that + tile + ov)].
 * Any out pointer may be NULL.  AT_ERR_ARG for a negative length and a bad tile_cols, AT_ERR_DOMAIN for the scoring or the query. */
int at_scan_local_plan(int32_t len1, int32_t len2, int use_cutoff, int32_t cutoff, int32_t tile_cols, int m, int u, int o, int e,
                       int32_t *tile, int32_t *overlap, int64_t *ntiles, int64_t *nfull);
/* Host helper: ws of a hit of at_scan_local that ends in (end_i, end_j) with this score -- its alignment lies in the target columns
 * (ws, end_j]; a multiple of 16 */
int64_t at_scan_local_window(int32_t end_i, int64_t end_j, int32_t score, int m, int u, int o, int e);

/*
 * End-to-end affine alignment of reads against LONG targets: what at_search_strands(AT_MODE_FIT) delivers -- for each
 * query the best k hits (1 <= k <= 64) over the targets, one per (query, strand, target), a hit being exactly what
 * at_align_batch(AT_MODE_FIT) returns, use_jump off, for (query or its reverse complement, target): the whole query, both ends of the
 * target free, affine gaps; the score, the end cell (l1, j*) and the start state AT_ST_MID or AT_ST_LOW (M before L at equal score,
 * then the smallest column; the target's last column is left out of the end scan) -- with no bound on the target length (any int32).
 * A target shorter than the query is no candidate, and that is no error.  A target is cut into overlapping tiles that are swept as
 * ordinary fit pairs by the batch kernels; the best over the tiles is exact for every pair that scores >= c = max(cutoff, lb),
 * lb = min(m, u) * l1 + o + e being a score every candidate reaches (without a cutoff every pair is exact; the other pairs are no hits
 * under the cutoff anyway).
 *   domain: the handle's scoring with m >= 1, o <= -1, e <= -1 (u anything), use_jump off; queries of 1 .. 1 024 bases; any alphabet
 *   at_search takes; one GPU
 *   rank: higher score first, then the smaller target index, then strand 0 before strand 1 (at_search_strands' order)
 *   out_target .. out_nhits as in at_search_strands; end_j is the ABSOLUTE column j* of the target
 *   tile_cols: the end columns a tile owns, a multiple of 16; 0 = the library's default (1 024).  The results do not depend on it
 *   the four CIGAR outputs are either all NULL or laid out as in at_scan (an unused entry: 0 runs, a row of -1, no room).  The ops of a
 *   hit are those of the reference's walk on the full table; AT_CG_START_J is absolute.  They are made in a window of the target, and
 *   a window that does not reproduce its hit's score, state and end column is AT_ERR_RANGE, never a silent result
 * at_set_min_score and the edit settings neither matter nor change.  Synchronous.  nq == 0 writes nothing; nt == 0 gives every query 0
 * hits.  AT_ERR_DOMAIN: the scoring, use_jump set (site lists are per-target columns), an empty or too long query, a handle of a
 * multi-process job, a candidate pair on which fit is not defined (a query of one base against a target of one base);
 * AT_ERR_ARG: k outside 1..64, strands outside 1..3, tile_cols negative or no multiple of 16.  AT_ERR_RANGE, before anything is swept:
 * a tile is a pair of the batch entry and has its exact-score bound, max(|m|,|u|,|o|,|e|,|j|) * (l1 + min(longest target, T + ov) + 2)
 * < 2^24 with ov = round16up(l1 + floor((max(m,u) * l1 - c) / min(|o|,|e|)) + 1).
 * at_last_config: "scan-fit: tile=T overlap=OV tiles=N strands=fwd|rev|both, B blocks, S slices, k=K; " + the first slice's sweep text
 * + " sweep=..ms" (the device time of the sweep phase, as at_scan reports it) and, with CIGARs, "; windows: " and the window pass's
 * text.  OV is the largest overlap of the call's query lengths.
 */
int at_scan_fit(at_handle *h,
                int64_t nq, const uint8_t *q_blob, const int64_t *q_off, const int32_t *q_len,
                int64_t nt, const uint8_t *t_blob, const int64_t *t_off, const int32_t *t_len,
                int k, int use_cutoff, int32_t cutoff, int strands, int32_t tile_cols, int flags,
                int32_t *out_target, int32_t *out_score, int32_t *out_end_i, int32_t *out_end_j,
                int32_t *out_state, int32_t *out_strand, int32_t *out_nhits,
                int32_t *out_stats, int32_t *out_ncigar, int64_t *out_cigar_off,
                uint32_t *out_cigar, int64_t cigar_cap);
/* Host helper (no handle, no GPU): how at_scan_fit cuts a pair of len1 x len2 under the scoring m / u / o / e -- *tile = the end columns
 * a tile owns (tile n: n tile <= j < (n + 1) tile), *overlap = ov, the columns in front of them, *ntiles = ceil(len2 / tile), or 0 for
 * len2 < len1, *nfull = the leading tiles of the full shape len1 x (tile + ov).  Tile n sweeps the columns (max(0, n tile - ov),
 * min(len2, that + tile + ov)]; the tiles 1 .. min(ntiles - 1, ov / tile) would repeat tile 0's sweep and are not swept.  Any out
 * pointer may be NULL.  AT_ERR_ARG for a negative length and a bad tile_cols, AT_ERR_DOMAIN for the scoring, the query, or
 * tile + ov >= 2^31. */
int at_scan_fit_plan(int32_t len1, int32_t len2, int use_cutoff, int32_t cutoff, int32_t tile_cols, int m, int u, int o, int e,
                     int32_t *tile, int32_t *overlap, int64_t *ntiles, int64_t *nfull);
/* Host helper: the window (*ws, *we] of a hit of at_scan_fit that ends in column end_j with this score -- the fit pair (query, target
 * columns (ws, we]) has the hit's score and state, the end column end_j - ws and its ops; ws is a multiple of 16,
 * ws <= end_j < we <= len2 and we - ws >= len1.  AT_ERR_DOMAIN for the scoring or the query, AT_ERR_ARG for len2 < len1 or an end_j
 * outside 0 .. len2 - 1. */
int at_scan_fit_window(int64_t end_j, int32_t score, int32_t len1, int32_t len2, int m, int u, int o, int e, int64_t *ws, int64_t *we);

/*
 * EVERY occurrence of a read under a distance cutoff: at_scan keeps one hit per (query, strand, target); this entry
 * reports every one.  For a query of l1 >= 1 bases, a target of l2 bases and max_dist >= 0 let c = min(max_dist, l1 - 1) (a match
 * must cost less than deleting the whole read; a query of length 0 has no hits) and D the table of at_scan, D(0,j) = 0, D(i,0) = i.
 *   occurrence  column a >= 1 with v = D(l1,a) is an OCCURRENCE iff v <= c, D(l1,a-1) > v and, with b the last column of the run of
 *               columns a..b that all hold v, b == l2 or D(l1,b+1) > v: the leftmost column of each strict local minimum of the last
 *               row, plateaus included (the "first column wins" choice of at_scan and of the local arg-max)
 *   separation  with min_sep = s > 0 an occurrence (a, v) of a (query, strand, target) is reported iff no OTHER OCCURRENCE (a', v') of
 *               the same triple with |a - a'| <= s has (v', a') < (v, a) lexicographically.  s = 0 reports every occurrence;
 *               s = AT_SCAN_SEP_READ (-1) stands for each query's own length.  A window minimum, not a greedy chain: a hit may be
 *               dropped by a neighbour that is itself dropped, which makes the result independent of any processing order
 *   hit         target, strand (0 = the query as given, 1 = its reverse complement), distance v, end cell (l1, a) with a the
 *               ABSOLUTE column, state AT_ST_MID.  Its ops are those of at_scan's three-way rule walked on the full table from
 *               (l1, a); AT_CG_START_J is absolute
 *   order       the hits of a query by distance, then target index, then strand 0 first, then column (at_scan's rank, extended)
 * out_hit_off (nq + 1 entries) is ALWAYS complete: the hits of query q are the entries [out_hit_off[q], out_hit_off[q + 1]).  If
 * out_hit_off[nq] > hit_cap nothing else is written and the call returns AT_OK: the caller calls again with room.  Otherwise
 * out_target / out_score / out_end_j / out_strand (hit_cap entries each; out_strand may be NULL for AT_STRAND_FWD) hold the hits,
 * and the four CIGAR outputs, all NULL or all given, are laid out over the hits as in at_align_batch_cigar (out_stats 8 per hit,
 * out_cigar_off out_hit_off[nq] + 1 entries, words of the hits that end within cigar_cap; flags: AT_CIGAR_M or 0).
 *   tile_cols   as at_scan; the results do not depend on it
 *   cand_cap    the candidate records (12 bytes each, descents of the last row at or under c) a slice of pairs may leave on the
 *               device; 0 = the library's default (2^20, or the columns of the slice if that is less).  A slice with more is swept
 *               once more into a buffer of the counted size: the results do not depend on it.  AT_ERR_NOMEM only if that
 *               allocation fails
 * Queries of up to 1 024 bases, pure ACGT, u == 1; one GPU; synchronous.  The handle's at_set_edit_infix / at_set_edit_traceback
 * settings neither matter nor change.  AT_ERR_DOMAIN as at_scan; AT_ERR_ARG as at_scan and for max_dist < 0, min_sep < -1,
 * cand_cap < 0, hit_cap < 0.  at_last_config: "scan-hits: tile=T overlap<=OV groups=G max_dist=D min_sep=S strands=fwd|rev|both,
 * B blocks, S slices, candidates=N kept=M resweeps=R; myers-scan-hits bits=2 words/lane=W ..." and, with CIGARs, "; windows: " and
 * the window pass's text.
 */
#define AT_SCAN_SEP_READ (-1)
int at_scan_hits(at_handle *h,
                 int64_t nq, const uint8_t *q_blob, const int64_t *q_off, const int32_t *q_len,
                 int64_t nt, const uint8_t *t_blob, const int64_t *t_off, const int32_t *t_len,
                 int32_t max_dist, int32_t min_sep, int strands, int32_t tile_cols, int64_t cand_cap, int flags,
                 int64_t hit_cap, int64_t *out_hit_off,
                 int32_t *out_target, int32_t *out_score, int32_t *out_end_j, int32_t *out_strand,
                 int32_t *out_stats, int32_t *out_ncigar, int64_t *out_cigar_off, uint32_t *out_cigar, int64_t cigar_cap);

/*
 * All-vs-all of which only the pairs over a threshold leave the device: the overlap stage of an assembler wants
 * the few pairs of a read set that overlap, not the dense triangle of scores.  The pairs, their order and s1 = read a, s2 = read b
 * (a < b) are those of at_align_allpairs; so are the modes and their refusals (fit: AT_ERR_ARG; edit under at_set_edit_infix:
 * AT_ERR_DOMAIN).  A HIT is a pair of [first_pair, first_pair + npairs) whose exact score is >= threshold -- with AT_MODE_EDIT,
 * whose distance is <= threshold (the cutoff convention of at_search).  Per hit: out_pair its triangle index, out_a / out_b the two
 * reads, and score, end cell and state exactly as at_align_allpairs returns them for that pair.  The hits come in ascending pair
 * order, whatever chunk_pairs is (pairs per slice; <= 0: the default of at_align_allpairs_stream).
 *   capacity    *out_nhits is ALWAYS complete.  If it exceeds hit_cap nothing else is written and the call returns AT_OK: the caller
 *               calls again with room (the protocol of at_scan_hits).  Otherwise the seven per-hit arrays (hit_cap entries each)
 *               hold the hits
 *   CIGARs      the four CIGAR outputs are all NULL or all given and laid out over the hits as in at_align_batch_cigar: out_stats 8
 *               per hit, out_cigar_off *out_nhits + 1 entries, the words of the hits that end within cigar_cap; flags: AT_CIGAR_M
 *               or 0.  The alignments come from a second, traceback pass over the hits only; a pair whose second pass does not
 *               reproduce its score and end cell makes the call AT_ERR_RANGE.  With AT_MODE_EDIT they must be NULL (AT_ERR_ARG)
 *   the bound   with AT_MODE_OVERLAP the call engages the bit-parallel bound of at_set_min_score with `threshold` for its duration --
 *               pairs proven below it are not swept -- and puts the handle's own setting back.  Where the bound does not apply
 *               (reads over 1 024 bases, reads that need 8-bit words, scoring outside m >= 0, 2 c > m) every pair is swept
 * Per slice only a count and the kept records cross the link.  One GPU (a handle of a multi-process job: AT_ERR_DOMAIN);
 * synchronous.  A pair outside the reference's domain makes the call AT_ERR_DOMAIN; the text names the smallest such pair index.
 * AT_ERR_ARG also for hit_cap < 0, cigar_cap < 0, other flags.  at_last_config: "allpairs-hits: threshold=T, S slices of <= C
 * pairs, kept=M; " and the first slice's sweep text; with CIGARs "; alignments: " and the traceback pass's text follow.
 * Not here: reverse-complement or swapped orientations, several GPUs, CIGARs of edit distances, fit.
 */
int at_allpairs_hits(at_handle *h, int mode, int64_t nreads,
                     const uint8_t *seq_blob, const int64_t *off, const int32_t *len,
                     int64_t first_pair, int64_t npairs, int32_t threshold, int64_t chunk_pairs, int flags,
                     int64_t hit_cap, int64_t *out_nhits,
                     int64_t *out_pair, int32_t *out_a, int32_t *out_b,
                     int32_t *out_score, int32_t *out_end_i, int32_t *out_end_j, int32_t *out_state,
                     int32_t *out_stats, int32_t *out_ncigar, int64_t *out_cigar_off,
                     uint32_t *out_cigar, int64_t cigar_cap);

/*
 * Multi-process batches: one process per GPU, each with its own handle.  The pairs are independent, so
 * the only communication is a broadcast of rank 0's scoring block and a gather of results, both RCCL collectives on the
 * handles' devices (over xGMI inside a node).  `dir` is a directory all ranks can reach: rank 0 leaves the RCCL id there.
 * RCCL is loaded at at_comm_init, not linked.  at_comm_allgather gathers a different number of bytes from every rank:
 * sizes first, then one payload padded to the largest (the two-phase CIGAR gather); every rank receives everything.
 */
int at_comm_init(at_handle *h, int rank, int world, const char *dir);
int at_comm_broadcast_scoring(at_handle *h);
int at_comm_allgather(at_handle *h, const void *mine, int64_t mine_bytes, void *all, int64_t all_cap, int64_t *bytes_of_rank);
void at_comm_destroy(at_handle *h);
/* 1 if the library's hand-written RCCL declarations were checked against the installed <rccl/rccl.h> when it was built
 * (static_asserts in csrc/at_comm.hip: id size, enum values, every entry point's argument list), 0 if no header was there */
int at_comm_abi_checked(void);

/* Host helper: pack `npairs` pairs of raw bytes into the word layout above.
 * bits = 0 picks 2 when every byte is one of ACGT, else 8; the choice is
 * returned in *bits_out.  words_out must hold at_pack_words(...) int32s. */
int64_t at_pack_words(int64_t npairs, const int32_t *len1, const int32_t *len2, int bits);
int at_pack_batch(int64_t npairs, const uint8_t *seq_blob,
                  const int64_t *off1, const int32_t *len1,
                  const int64_t *off2, const int32_t *len2,
                  int bits, int *bits_out,
                  uint32_t *words_out, int64_t *woff1_out, int64_t *woff2_out);

/* Host helper: ops (END -> START) + end cell -> the reference's two gapped
 * strings (what trace_back_* + strrev produce).  r1/r2 need nops+1 bytes. */
int at_render(const uint8_t *ops, int32_t nops,
              const uint8_t *s1, int32_t end_i, const uint8_t *s2, int32_t end_j,
              char *r1, char *r2);

/* Introspection for benchmarks / tests: name of the kernel configuration the
 * last batch ran with ("small"/"large", bits, waves), never NULL. */
const char *at_last_config(const at_handle *h);

#ifdef __cplusplus
}
#endif
#endif /* ALIGNTOOLS_HIP_H */
