/*
 * hypmerge.h -- C ABI of libhypmerge.so, the MI355X (gfx950) merge engine for HypTokenizer.
 *
 * The reference (sangaprabhav/HypTokenizer) has no FFI / plugin interface on this path: the hot
 * path is plain Python calling PyTorch.  Each entry point below therefore
 * cites the reference PYTHON call site it replaces; INTEGRATION.md shows the ctypes binding a
 * maintainer of the reference would add at that site.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no torch / C++ types in any signature.
 *   - `*_dev` pointers are device addresses owned by the caller (e.g. tensor.data_ptr());
 *     all other pointers are host memory owned by the caller.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  Functions that return
 *     results in HOST memory synchronise that stream before returning; functions that only
 *     write device memory are asynchronous on it.
 *   - return value: 0 = HM_OK; negative = argument / capacity error (HM_E_*); positive = hipError_t.
 *     hm_last_error() returns a human-readable message for the last non-zero status.
 *   - table layout handed in by the caller is the reference's: row-major fp32 [n_rows, ld],
 *     column 0 = time coordinate, columns 1..d = spatial (tokenizer/hyperbolic_merge.py:145-153).
 *   - sign_mode: 0 = arithmetic of the reference as shipped (u = -minkowski_dot),
 *                1 = standard Lorentz sign (u = +minkowski_dot).
 *   - candidate order everywhere: ascending fp32 distance, ties by row-major (i, j)
 *     (stable sort of the nonzero() list, hyperbolic_merge.py:263-269,378; fast...:349-355,371).
 *   - every distance is d = acosh(max(u,1)) / sqrt(c) evaluated with the canonical fp32
 *     arithmetic of DESIGN.md; thresholds compare in fp32 (d < thr, NaN never passes).
 */
#ifndef HYPMERGE_H
#define HYPMERGE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HM_ABI_VERSION 3

#define HM_OK            0
#define HM_E_ARG        (-1)   /* bad argument (null pointer, range, unsupported dimension) */
#define HM_E_CAPACITY   (-2)   /* an internal workspace was too small for this request      */
#define HM_E_STATE      (-3)   /* call order violated (e.g. scan before hm_set_table)        */
#define HM_E_NOMEM      (-4)
#define HM_E_COMM       (-5)   /* RCCL could not be loaded / a collective failed            */
#define HM_E_NA         (-6)   /* the request does not apply to the engine's current state: an ordinary answer, no message */

#define HM_SIGN_REFERENCE 0
#define HM_SIGN_LORENTZ   1

/* form of the pair scan's MFMA prefilter (results are identical: every reported distance is re-evaluated in the
 * canonical fp32 arithmetic): AUTO = bf16 MFMA from d >= 24, else fp32 MFMA */
#define HM_PREFILTER_AUTO 0
#define HM_PREFILTER_F32  1
#define HM_PREFILTER_BF16 2

typedef struct hm_engine hm_engine;

int         hm_abi_version(void);
const char* hm_last_error(const hm_engine* e);          /* e may be NULL: last global error */

/* One engine per device.  Allocates the scan image ([max_rows] rows) and all workspaces; nothing
 * is allocated in the per-call path afterwards.
 * LIMITS (narrower than the reference, which takes any max_vocab_size; both are rejected here with HM_E_ARG, by the Python
 * classes at construction with a ValueError):
 *   2 <= max_rows <= 1048576  -- the pair scan's 64-bit argmin running key packs (i, j) into 32 bits with ib row-index bits,
 *                                ib = max(17, ceil(log2(max_rows))): (i << (32 - ib)) | (j >> (2 ib - 32)).  Up to 131072
 *                                rows that is the narrow key (i << 15) | (j >> 2); larger engines use the wide form, which
 *                                only lets more zero-distance ties through to the exact re-evaluation;
 *   2 <= d1 = d + 1 <= 129    -- kernels are instantiated for d <= 128; the bf16 prefilter exists for d <= 124 (d + 4 K-slots
 *                                in at most 16 chunks of 8), wider tables use the fp32 prefilter.
 * Replaces: the pre-allocated table of HyperbolicTokenizer.__init__ (hyperbolic_merge.py:144-153)
 * as far as the search kernels are concerned, and the FAISS index objects
 * (_init_faiss_index :593-605, _build_faiss_index fast...:195-240), which are not used at all. */
int hm_engine_create(hm_engine** out, int device, int64_t max_rows, int d1, int sign_mode, int prefilter);
int hm_engine_destroy(hm_engine* e);
/* Change the prefilter form of a live engine (HM_PREFILTER_*).  The environment variable HM_SCAN_PRECISION
 * ("f32" | "bf16") overrides the argument of hm_engine_create, not this call. */
int hm_set_prefilter(hm_engine* e, int prefilter);

/* (Re)build the scan image from rows [0, n_rows) of the caller's table.  Replaces nothing in the
 * reference (it re-reads self.embeddings[:n] every step, hyperbolic_merge.py:250). */
int hm_set_table(hm_engine* e, const float* X_dev, int64_t ld, int64_t n_rows, void* stream);
/* Refresh image rows [row_begin, row_end) after the caller changed those table rows. */
int hm_update_rows(hm_engine* e, const float* X_dev, int64_t ld, int64_t row_begin, int64_t row_end,
                   void* stream);
int64_t hm_rows(const hm_engine* e);                     /* live rows in the image */

/* K1: nearest pair.  Over all pairs i<j<n with row_begin <= i < row_end: the smallest (d, i, j)
 * with d < thr.  *found = 0 when no pair qualifies.  Results in host memory.
 * Replaces: _find_merge_candidates + sort + [0] of HyperbolicTokenizer.optimize_merges
 * (hyperbolic_merge.py:371-396, candidate search :247-269). */
int hm_pairwise_argmin(hm_engine* e, float c, float thr, int64_t row_begin, int64_t row_end,
                       float* d, int32_t* i, int32_t* j, int32_t* found, void* stream);

/* K1, device-resident form for the multi-GPU exchange: same search, but the 16-byte record
 * {found, bits(d), i, j} (uint32 x 4; found = 2 means "emission buffer overflowed, call the host
 * form") is written to rec_dev and nothing is synchronised -- the record can feed an RCCL
 * all-gather on the same stream directly. */
int hm_pairwise_argmin_dev(hm_engine* e, float c, float thr, int64_t row_begin, int64_t row_end,
                           uint32_t* rec_dev, void* stream);

/* K2: the k smallest candidates in order, and the exact number of candidates.
 * d_out/i_out/j_out have room for k entries (may be NULL when k == 0); *n_out = min(k, *count).
 * Replaces: the recompute branch of _find_merge_candidates_fast + candidates.sort() +
 * AdaptiveMergeCache.add_batch truncation to max_size (fast_hyperbolic_merge.py:336-355,371-374,78-95).
 * Always answers for k <= 65536, at any pair count: a table whose distances are so concentrated that no emission cut of the matrix-core
 * prefilter fits the engine's buffers (all u within a few hundred ulps of 1) is searched by evaluating every pair in the
 * canonical arithmetic and selecting by counting (hm_exact.hip) -- like the reference, only slower than the usual path
 * (56 ms at 25 000 rows).  The same holds for hm_pairwise_argmin, hm_pairwise_topk_nocount and hm_pairwise_count. */
int hm_pairwise_topk(hm_engine* e, float c, float thr, int64_t k, int64_t row_begin, int64_t row_end,
                     float* d_out, int32_t* i_out, int32_t* j_out, int64_t* n_out, int64_t* count,
                     void* stream);

/* K2 without the exact total: the same ordered k smallest candidates; *count is the exact number of candidates
 * when fewer than k exist, else -1 ("at least k, not counted" -- the scan then visits only what lies below its
 * emission cut; hm_pairwise_count delivers the number when a caller asks for it).  The reference consumes the
 * total only in log lines (fast_hyperbolic_merge.py:521,526) and for emptiness (:529). */
int hm_pairwise_topk_nocount(hm_engine* e, float c, float thr, int64_t k, int64_t row_begin, int64_t row_end,
                             float* d_out, int32_t* i_out, int32_t* j_out, int64_t* n_out, int64_t* count, void* stream);
/* The same refresh in two halves for callers that have host work to do meanwhile (the fast tokenizer's string
 * bookkeeping): hm_topk_refresh_begin enqueues the whole chain and returns at once -- HM_E_NA when
 * the refresh is not of the incremental kind (rows changed, other k / curvature, lower threshold: use
 * hm_pairwise_topk_nocount; HM_E_STATE stays a real error: a refresh already pending) --, hm_topk_refresh_end waits and delivers the ordered list (HM_E_CAPACITY: more new entries
 * than the device-side sort takes; the state is untouched, run hm_pairwise_topk_nocount).  No other call on the engine in
 * between. */
int hm_topk_refresh_begin(hm_engine* e, float c, float thr, int64_t k, void* stream);
int hm_topk_refresh_end(hm_engine* e, float* d_out, int32_t* i_out, int32_t* j_out, int64_t* n_out);
/* Exact number of candidates among the first n_limit rows (n_limit < 0: all live rows).  Rows are only ever
 * appended, so this is len(candidates) of the search that ran when the table had n_limit rows. */
int hm_pairwise_count(hm_engine* e, float c, float thr, int64_t n_limit, int64_t* count, void* stream);

/* All candidates (unordered) -- the caller sorts them row-major.  min(cap, *total) triples are written;
 * *total is the exact number (also past the emission buffer: the triples are then taken from the first rows).  Replaces: the candidate list of _find_merge_candidates
 * (hyperbolic_merge.py:247-269) when a caller really wants every tuple. */
int hm_pairwise_candidates(hm_engine* e, float c, float thr, int64_t row_begin, int64_t row_end,
                           int64_t cap, int32_t* i_out, int32_t* j_out, float* d_out, int64_t* total,
                           void* stream);

/* K3: distances from image row `row` to image rows [0, n): d_out_dev[n] (device).
 * No reference equivalent (incremental maintenance). */
int hm_row_vs_all(hm_engine* e, int64_t row, int64_t n, float c, float* d_out_dev, void* stream);

/* K3 + reduction: the nearest partner of image row `row` among rows [0, n_partners) (itself
 * excluded): smallest (d, min(i,row), max(i,row)) with d < thr, in host memory.  Lets a caller
 * maintain the global nearest pair incrementally: rows are only ever appended, so after
 * a merge the global minimum is min(previous minimum, nearest partner of the new row).
 * No reference equivalent (the reference recomputes everything, hyperbolic_merge.py:247-269). */
int hm_row_argmin(hm_engine* e, int64_t row, int64_t n_partners, float c, float thr, float* d, int32_t* i,
                  int32_t* j, int32_t* found, void* stream);

/* K5: gathered pair distances on the image: out_dev[t] = d(row I[t], row J[t]).
 * Replaces: distance(...).item() loops (_compute_distance_statistics fast...:448-455,
 * n<=100 branch hyperbolic_merge.py:270-289). */
int hm_pair_distance(hm_engine* e, const int32_t* I_dev, const int32_t* J_dev, int64_t b, float c,
                     float* out_dev, void* stream);

/* K4: batched "midpoint" project(exp_map(x_i, w * log_map(x_i, x_j))) on the image rows,
 * out_dev[b, d1] in the reference's column order.
 * Replaces: _merge_tokens arithmetic (hyperbolic_merge.py:326-340) and the loop of
 * _evaluate_candidates_parallel (:568-587). */
int hm_midpoint_batch(hm_engine* e, const int32_t* I_dev, const int32_t* J_dev, const float* W_dev,
                      int64_t b, float c, float* out_dev, void* stream);

/* Fused merge step: midpoint of image rows (i, j) with weight w is written to row `new_row` of the
 * caller's table AND of the image; the live-row count becomes max(rows, new_row + 1).
 * Replaces: hyperbolic_merge.py:326-351 (log_map, scale, exp_map, project, embeddings.data[n] = x). */
int hm_merge_append(hm_engine* e, int32_t i, int32_t j, float w, float c, float* X_dev, int64_t ld,
                    int64_t new_row, void* stream);

/* Several merges known in advance, one launch: merge t = midpoint of image rows (I[t], J[t]) with weight W[t] ->
 * row first_row + t of the table and of the image.  independent = 0: a merge may read rows written by earlier merges
 * of the batch (sequential chain); independent = 1: the caller guarantees every I[t], J[t] < first_row (all at once).
 * Replaces: the hyperbolic_merge.py:326-351 arithmetic of the ~100 merges a FastHyperbolicTokenizer performs
 * between two refreshes (fast_hyperbolic_merge.py:546-549), all of which are known when the refresh returns. */
int hm_merge_append_batch(hm_engine* e, const int32_t* I_dev, const int32_t* J_dev, const float* W_dev, int64_t count,
                          float c, float* X_dev, int64_t ld, int64_t first_row, int independent, void* stream);
/* The same with I / J / W in HOST memory (at most 4096 merges): staged through the engine's pinned buffer. */
int hm_merge_append_batch_host(hm_engine* e, const int32_t* I_host, const int32_t* J_host, const float* W_host, int64_t count,
                               float c, float* X_dev, int64_t ld, int64_t first_row, int independent, void* stream);
/* Forget image rows >= n_rows (undo rows appended ahead of time). */
int hm_truncate(hm_engine* e, int64_t n_rows, void* stream);

/* ---- device-resident merge loops ------------------------------------------------------------------------
 * Token lengths len(vocab[r]) for rows [0, n): the only thing a merge needs from the token strings
 * (w = len(tj) / (len(ti) + len(tj)), hyperbolic_merge.py:317-323).  Host array; kept on the device and
 * extended by the loops below (len[new] = len[i] + len[j]). */
int hm_set_token_lengths(hm_engine* e, const int32_t* lens_host, int64_t n, void* stream);
/* `steps` (<= 256) iterations of HyperbolicTokenizer.optimize_merges (hyperbolic_merge.py:371-399: full search,
 * sort, [0], merge) enqueued back to back -- pair scan + one tail kernel per step, no host round trip -- and read
 * back with one synchronisation.  rec_out[4 * k] = {found, bits(d), i, j} of step k: found 1 = merged (i, j) into
 * row n + k; 0 = no candidate (the loop ends, hyperbolic_merge.py:373-375); 2 = emission overflow at this step (run it
 * through hm_pairwise_argmin + hm_merge_append); 3 = skipped after a 0 / 2.  *done = leading merged steps. */
int hm_std_merge_steps(hm_engine* e, float c, float thr, float* X_dev, int64_t ld, int64_t steps, uint32_t* rec_out,
                       int64_t* done, void* stream);
/* The same merges with the nearest pair maintained as a running minimum (rows are only appended):
 * one launch per step (merge + new row vs all rows + fold).  best_io = {found, bits(d), i, j}: in: the nearest
 * pair of the current table (from hm_pairwise_argmin); out: the running minimum after the last executed step. */
int hm_incr_merge_steps(hm_engine* e, float c, float thr, float* X_dev, int64_t ld, int64_t steps, uint32_t* best_io,
                        uint32_t* rec_out, int64_t* done, void* stream);

/* The same loop row-sharded over ranks, without a host round trip per step.  Between
 * hm_shard_loop_begin and hm_shard_loop_end the caller enqueues, per step: hm_pairwise_argmin_dev over the rank's row
 * range -> an all-gather of the ranks' 16-byte records on the same stream (RCCL) -> hm_shard_merge_step, which takes the
 * lexicographic minimum of the `world` (<= 64) gathered records (identical on every rank) and applies the merge to this
 * rank's replica (row = current row count, weights from the token lengths), or ends the loop on the device: no pair
 * anywhere (record found = 0), an emission overflow on some rank (found = 2: the caller runs that step through the
 * bounded host path); later steps of the batch then skip themselves (found = 3).  hm_shard_loop_end synchronises once
 * and returns the step records as hm_std_merge_steps does. */
int hm_shard_loop_begin(hm_engine* e, void* stream);
int hm_shard_merge_step(hm_engine* e, const uint32_t* recs_dev, int world, float c, float* X_dev, int64_t ld, int64_t step,
                        void* stream);
int hm_shard_loop_end(hm_engine* e, int64_t steps, uint32_t* rec_out, int64_t* done, void* stream);

/* ---- the exchange step inside the library (hm_comm_init, hm_global_argmin, hm_global_topk) ----
 * One process per GPU; every rank holds a replica of the table and an engine of its own.  hm_comm_unique_id (one rank)
 * produces the 128-byte RCCL id the host program hands to the other ranks by its own means (torch.distributed broadcast,
 * MPI, a file); hm_comm_init binds an RCCL communicator (over xGMI on one node) to the engine; collective calls below must
 * then be made by every rank with the same arguments.  librccl.so.1 is bound at run time (the copy already loaded by the
 * process when there is one): HM_E_COMM when it is missing.  Rows are cut into `world` ranges of equal pair count.
 * Replaces: nothing in the reference (single process); the loop sharded is hyperbolic_merge.py:357-412. */
#define HM_COMM_ID_BYTES 128
int hm_comm_unique_id(void* id_out128);
int hm_comm_init(hm_engine* e, const void* id128, int rank, int world);
int hm_comm_destroy(hm_engine* e);
int hm_comm_info(const hm_engine* e, int* rank, int* world);          /* rank = -1, world = 0 without a communicator */
/* `steps` (<= 256) iterations of the standard loop, row-sharded, enqueued from the library with no host code per step:
 * scan of this rank's rows -> record -> ncclAllGather (16 bytes per rank) -> global minimum + merge into this rank's
 * replica.  Records / *done as hm_std_merge_steps (identical on every rank). */
int hm_shard_merge_steps(hm_engine* e, float c, float thr, float* X_dev, int64_t ld, int64_t steps, uint32_t* rec_out,
                         int64_t* done, void* stream);
/* C1: the global nearest pair (search of this rank's rows, all-gather of the records, minimum).  Host results. */
int hm_global_argmin(hm_engine* e, float c, float thr, float* d, int32_t* i, int32_t* j, int32_t* found, void* stream);
/* C2: the k smallest candidates of the whole table in order and their exact number: every rank's ordered list of its rows
 * stays on the device, the lists are all-gathered and merged there by the exact selection (no host round trip of the
 * lists).  Arguments as hm_pairwise_topk without the row range. */
int hm_global_topk(hm_engine* e, float c, float thr, int64_t k, float* d_out, int32_t* i_out, int32_t* j_out, int64_t* n_out,
                   int64_t* count, void* stream);

/* Measurement aid: with on != 0, hm_std_merge_steps records a HIP event pair around every scan launch of a batch (all of
 * them enter hm_scan_totals) and around the whole batch; hm_last_loop_timing returns the last batch's wall time on the
 * device, the sum of its scan launches and its step count (0 when the batch stopped early). */
int hm_debug_time_loops(hm_engine* e, int on);
int hm_last_loop_timing(hm_engine* e, float* batch_ms, float* scan_ms, int64_t* steps);

/* ---- enhanced tokenizer (BASELINE config 5) ---------------------------------------------------------------
 * Semantic-coherence distances: for candidate t the simulated merged embedding
 * m = exp_map(x_I[t], W[t] * log_map(x_I[t], x_J[t])) -- NOT projected -- and out_dev[t * ns + s] =
 * distance(m, x_S[t * ns + s]).  Sampling, the skip of s in {i, j}, mean and sigmoid stay with the caller.
 * Replaces: the loop of tokenizer/enhanced_fast_hyperbolic_merge.py:308-333 (one midpoint + <= 50
 * distance().item() calls per candidate). */
int hm_coherence_batch(hm_engine* e, const int32_t* I_dev, const int32_t* J_dev, const float* W_dev, const int32_t* S_dev,
                       int64_t b, int ns, float c, float* out_dev, void* stream);
/* project_to_hyperboloid over rows [0, n_rows) of the caller's table IN PLACE (only column 0 changes) and the
 * matching refresh of the engine's images and norm bounds for the live rows.  n_rows >= live rows.
 * Replaces: _project_embeddings (enhanced_fast_hyperbolic_merge.py:784-792) and the constructor's :243-244. */
int hm_project_table(hm_engine* e, float* X_dev, int64_t ld, int64_t n_rows, float c, void* stream);

/* Host-only helper (no GPU work): out[t * ns + q] = torch.randperm(n)[q] for t = 0..count-1 and q < ns, drawn from
 * the MT19937 state of torch's CPU generator -- mt_state[624] words, *left, *next as in at::mt19937 -- which is
 * advanced exactly as `count` calls of torch.randperm(n) would advance it (n < 2^32 / 20, ns <= 4096).
 * Replaces: torch.randperm(current_vocab_size)[:sample_size] per scored candidate
 * (enhanced_fast_hyperbolic_merge.py:324-325): O(n) draws of the recurrence instead of an O(n) random-access shuffle. */
int hm_randperm_prefix(uint32_t* mt_state, int32_t* left, uint32_t* next, int64_t n, int32_t ns, int64_t count, int32_t* out);

/* ---- batch tokenizer ---------------------------------------------------------------
 * HyperbolicTokenizer.tokenize for many lines at once, over 32-bit symbols: the caller maps every distinct
 * string (characters, rule operands, rule results) to a symbol >= 0 and any other character to a NEGATIVE
 * symbol (never matches a rule, passes through).  Semantics are the reference's positional fixed point:
 * repeated left-to-right passes, a hit replaces tokens[i] by the rule's result, removes tokens[i+1] and stays
 * at i, until a pass changes nothing.
 * Replaces: tokenizer/hyperbolic_merge.py:414-446 (and with it encode :448-459) as driven per line by
 * scripts/benchmark_efficiency.py:58-94.
 *
 * Symbols of rules lie in [0, 2^21 - 1) (two million distinct strings).
 *
 * hm_tokenize_table_capacity / hm_tokenize_build_table are host-only: they build the open-addressing rule table
 * {(left, right) -> merged} as `capacity` 8-byte entries left:21 | right:21 | merged+1:22 in buckets of two (a later
 * rule for the same pair replaces the earlier one, as dict assignment does, :425-428); the caller copies the
 * `capacity` words to 16-byte-aligned device memory. */
int64_t hm_tokenize_table_capacity(int64_t n_rules);
int hm_tokenize_build_table(const int32_t* left, const int32_t* right, const int32_t* merged, int64_t n_rules,
                            uint64_t* table_out, int64_t capacity);
/* sym_dev: symbols of all lines concatenated (each line < 2^31 symbols); offsets_dev[n_lines + 1]; order_dev:
 * optional permutation of the lines (lane t handles line order_dev[t]; longest-first keeps the 64 lines of a wave
 * alike), may be NULL.  Line l's tokens are written to out_dev[offsets[l] .. offsets[l] + out_len_dev[l]);
 * passes_dev (optional) receives the number of passes the reference's while-loop runs.  Asynchronous on `stream`. */
int hm_tokenize_batch(const int32_t* sym_dev, const int64_t* offsets_dev, const int64_t* order_dev, int64_t n_lines,
                      const uint64_t* table_dev, int64_t capacity, int32_t* out_dev, int32_t* out_len_dev,
                      int32_t* passes_dev, void* stream);

/* ---- token statistics of a tokenised corpus (corpus metrics of a tokenizer) ----------------------------------
 * The integer counts behind the reference's corpus evaluation, over the token stream exactly as hm_tokenize_batch
 * leaves it: line l is tok_dev[offsets_dev[l] .. offsets_dev[l] + len_dev[l]) (offsets_dev[0] = 0, n_positions =
 * offsets_dev[n_lines]); the slots behind a line's tokens, up to offsets_dev[l + 1], are never read as tokens.
 * Replaces: the token loops of scripts/compare_tokenizers.py -- benchmark_hyperbolic_tokenizer :177-185 (tokens and their
 * characters), evaluate_linguistic_quality :254-278 (word-boundary, morpheme and sub-word counts) and
 * evaluate_compression_efficiency :311-320 -- and the per-line loop of scripts/benchmark_efficiency.py:58-94.
 *
 * attr_dev[n_sym] (n_sym <= 2^21): one word per symbol >= 0, built by the caller from the symbol's string:
 *   bit 0  HM_TOKSTATS_NONWORD     the string contains a character that is not a word character  (re: [^\w])
 *   bit 1  HM_TOKSTATS_MORPHEME    the string matches the reference's suffix pattern              (:250-252)
 *   bit 2  HM_TOKSTATS_FIRST_WORD  its first character is a word character
 *   bit 3  HM_TOKSTATS_LAST_WORD   its last character is a word character
 *   bits 4-7 zero;  bits 8-31: its length in code points (at most HM_TOKSTATS_MAX_LEN)
 * wordmap_dev: 0x110000 bits (34 816 words), bit cp & 31 of word cp >> 5 set when code point cp is a word character.  A
 * negative symbol -(2 + cp) is a token of length 1 with the flags of cp; it never matches the suffix pattern.  A symbol
 * that is neither (>= n_sym, -1, beyond the code space) counts as a token of length 0 without flags.
 *
 * totals_dev[HM_TOKSTATS_COUNTERS] (zeroed by the call): [0] tokens, [1] code points of the tokens, [2] tokens with a
 * non-word character, [3] tokens matching the suffix pattern, [4] sub-word tokens: token i of a line of n tokens whose
 * predecessor (i > 0) ends in, or whose successor (i < n - 1) starts with, a word character on the other side of a word
 * character of its own (:276-278); neighbours never cross a line.  line_counts_dev (may be NULL): the same five counts per
 * line, [n_lines][HM_TOKSTATS_COUNTERS], zeroed by the call.  Sums of integers: no result depends on the launch geometry.
 * The kernel works on tiles of HM_TOKSTATS_TILE positions; max_blocks (0: four per compute unit) caps the grid (tests).
 * HM_E_ARG (before any device is touched): a negative size, a NULL array that is needed, n_positions >= 2^40.
 * Asynchronous on `stream`; the current device must be the one holding the arrays. */
#define HM_TOKSTATS_COUNTERS 5
#define HM_TOKSTATS_NONWORD 1u
#define HM_TOKSTATS_MORPHEME 2u
#define HM_TOKSTATS_FIRST_WORD 4u
#define HM_TOKSTATS_LAST_WORD 8u
#define HM_TOKSTATS_LEN_SHIFT 8
#define HM_TOKSTATS_MAX_LEN ((1 << 24) - 1)
#define HM_TOKSTATS_TILE 1024
int hm_tokstats(const int32_t* tok_dev, const int64_t* offsets_dev, const int32_t* len_dev, int64_t n_lines,
                int64_t n_positions, const uint32_t* attr_dev, int64_t n_sym, const uint32_t* wordmap_dev,
                uint64_t* totals_dev, uint64_t* line_counts_dev, int64_t max_blocks, void* stream);

/* ---- greedy longest-match counter (compression-aware scoring) -----------------------------------------------
 * Token counts of a corpus sample under "vocabulary + one candidate string" for K candidates at once, by the
 * reference's greedy rule: at position p the longest vocabulary entry that is a prefix of text[p:], else text[p].
 * Everything is Unicode code points (int32, Python str positions).  Empty strings never match (the reference's loop
 * does not terminate on them).  Independent of any engine; errors are reported through hm_last_error(NULL).
 * Inputs are HOST arrays (strings as code points concatenated + int64 offsets[count + 1], offsets[0] = 0); outputs
 * are device arrays.  Every entry point synchronises `stream` before it returns.
 * LIMITS (HM_E_ARG): corpus code points < 2^31 and lines < 2^31; vocabulary pool < 2^31 code points; candidate code
 * points < 2^31, K < 2^31, lines * ceil(K / 64) < 2^31; every string shorter than 2^31; multiplicities >= 0.
 *
 * hm_greedy_create / hm_greedy_destroy: one matcher on device `device`.
 * Replaces: the per-instance tokenize_cache machinery of CompressionAwareTokenizer (compression_aware_tokenizer.py:84-87). */
typedef struct hm_greedy hm_greedy;
int hm_greedy_create(hm_greedy** out, int device);
int hm_greedy_destroy(hm_greedy* g);
/* The corpus: n_lines lines (representative texts), mult[n_lines] >= 0 their multiplicities.  Rebuilds lm (longest
 * vocabulary match per position) from every string added so far and the per-line base counts.
 * Replaces: the iteration over self.corpus_sample (compression_aware_tokenizer.py:152-161; enhanced...:884-891), with
 * lines that share their cache key merge_{i}_{j}_{text[:20]} folded into one line of multiplicity > 1. */
int hm_greedy_set_corpus(hm_greedy* g, const int32_t* cps, const int64_t* offsets, const int64_t* mult, int64_t n_lines,
                         void* stream);
/* Append vocabulary strings (the vocabulary only ever grows: vocab.append in _merge_tokens, hyperbolic_merge.py:343-355).
 * lm[p] = max(lm[p], |t|) wherever a new string t occurs; more than 64 strings at once rebuild lm through the hashed set.
 * Replaces: temp_vocab = self.vocab.copy() + sorted(vocab, key=len) per candidate (compression_aware_tokenizer.py:148-150,
 * :104-105). */
int hm_greedy_add_strings(hm_greedy* g, const int32_t* cps, const int64_t* offsets, int64_t n_strings, void* stream);
/* k candidate strings m_c: counts_dev[c * n_lines + l] (may be NULL) = greedy token count of line l under
 * vocabulary + {m_c}; totals_dev[c] = sum_l mult[l] * counts[c][l].  HM_E_STATE before hm_greedy_set_corpus.
 * Replaces: the per-candidate _tokenize_with_vocab loop (compression_aware_tokenizer.py:143-161, :91-120) and
 * _compute_compression_score's (enhanced_fast_hyperbolic_merge.py:849-899). */
int hm_greedy_count(hm_greedy* g, const int32_t* cps, const int64_t* offsets, int64_t k, int32_t* counts_dev,
                    int64_t* totals_dev, void* stream);
/* Copies of the matcher's lm[corpus code points] and base[n_lines] (either may be NULL).  No reference equivalent
 * (inspection: the incremental lm equals a rebuild). */
int hm_greedy_longest(hm_greedy* g, int32_t* lm_dev, int32_t* base_dev, void* stream);

/* Dense distance block between two arbitrary device arrays: out_dev[n1, n2].
 * Replaces: batch_distance / batch_distance_optimized (embedding/lorentz_model.py:141-210) and
 * _compute_pairwise_distances (hyperbolic_merge.py:166-190).  Engine-independent. */
int hm_batch_distance(const float* X_dev, int64_t n1, const float* Y_dev, int64_t n2, int64_t ld_x,
                      int64_t ld_y, int d1, float c, int sign_mode, float* out_dev, void* stream);

/* Row-wise Lorentz primitives on device arrays [b, d1] with leading dimension ld
 * (embedding/lorentz_model.py).  Engine-independent.
 *   hm_rows_minkowski : out[b]      = minkowski_dot(x, y)            (:14-25, sign_mode applies)
 *   hm_rows_distance  : out[b]      = distance(x, y, c)              (:122-138)
 *   hm_rows_log_map   : out[b, d1]  = log_map(x, y)                  (:96-119)
 *   hm_rows_exp_map   : out[b, d1]  = exp_map(x, v)                  (:73-93)
 *   hm_rows_project   : out[b, d1]  = project_to_hyperboloid(x, c)   (:41-56)           */
int hm_rows_minkowski(const float* x_dev, const float* y_dev, int64_t b, int64_t ld, int d1, int sign_mode,
                      float* out_dev, void* stream);
int hm_rows_distance(const float* x_dev, const float* y_dev, int64_t b, int64_t ld, int d1, float c,
                     int sign_mode, float* out_dev, void* stream);
int hm_rows_log_map(const float* x_dev, const float* y_dev, int64_t b, int64_t ld, int d1, int sign_mode,
                    float* out_dev, int64_t ld_out, void* stream);
int hm_rows_exp_map(const float* x_dev, const float* v_dev, int64_t b, int64_t ld, int d1, float* out_dev,
                    int64_t ld_out, void* stream);
int hm_rows_project(const float* x_dev, int64_t b, int64_t ld, int d1, float c, float* out_dev,
                    int64_t ld_out, void* stream);

/* Vector-Jacobian products of the row-wise primitives above (upstream gradient g, same row layout; outputs [b, d1] with
 * leading dimension ld_out).  The derivative is that of the reference's torch expression as torch differentiates it:
 * clamp(u, min = 1 + 1e-8) passes the gradient where u >= 1.0f and gives exactly 0 below; acosh' = 1 / sqrt(a^2 - 1) is
 * +-inf at a == 1; the mask arithmetic of log_map / exp_map is walked back term by term.  No gradient with respect to c.
 *   hm_rows_minkowski_bwd : g[b]            -> gx, gy     (:14-25)
 *   hm_rows_distance_bwd  : g[b]            -> gx, gy     (:122-138)
 *   hm_rows_log_map_bwd   : g[b, d1] (ld_g) -> gx, gy     (:96-119)
 *   hm_rows_exp_map_bwd   : g[b, d1] (ld_g) -> gx, gv     (:73-93)
 *   hm_rows_project_bwd   : g[b, d1] (ld_g) -> gx         (:41-56; column 0 of gx is 0)
 *   hm_batch_distance_bwd : G[n1, n2] (ld_g) -> gX[n1, d1], gY[n2, d1] (:141-210; either output may be NULL); every row
 *                           is summed over the other table's rows in ascending order, no atomics: same bits on every run */
int hm_rows_minkowski_bwd(const float* x_dev, const float* y_dev, const float* g_dev, int64_t b, int64_t ld, int d1,
                          int sign_mode, float* gx_dev, float* gy_dev, int64_t ld_out, void* stream);
int hm_rows_distance_bwd(const float* x_dev, const float* y_dev, const float* g_dev, int64_t b, int64_t ld, int d1,
                         float c, int sign_mode, float* gx_dev, float* gy_dev, int64_t ld_out, void* stream);
int hm_rows_log_map_bwd(const float* x_dev, const float* y_dev, const float* g_dev, int64_t ld_g, int64_t b, int64_t ld,
                        int d1, int sign_mode, float* gx_dev, float* gy_dev, int64_t ld_out, void* stream);
int hm_rows_exp_map_bwd(const float* x_dev, const float* v_dev, const float* g_dev, int64_t ld_g, int64_t b, int64_t ld,
                        int d1, float* gx_dev, float* gv_dev, int64_t ld_out, void* stream);
int hm_rows_project_bwd(const float* x_dev, const float* g_dev, int64_t ld_g, int64_t b, int64_t ld, int d1, float c,
                        float* gx_dev, int64_t ld_out, void* stream);
int hm_batch_distance_bwd(const float* X_dev, int64_t n1, const float* Y_dev, int64_t n2, int64_t ld_x, int64_t ld_y,
                          int d1, float c, int sign_mode, const float* G_dev, int64_t ld_g, float* gX_dev, float* gY_dev,
                          int64_t ld_out, void* stream);

/* Row-wise Poincare-ball primitives (embedding/poincare_ball.py of the reference) on device arrays [b, d] with leading
 * dimension ld, 1 <= d <= 128; the Lorentz side of the two conversions has d + 1 columns.  Engine-independent.  Every
 * call returns HM_E_ARG before touching the device for a NULL pointer, d out of range, a leading dimension below the row
 * width, or a c that is not finite and > 0.  Rows are read with 16-byte accesses when d, the leading dimensions and the
 * base addresses allow it.
 *   hm_rows_mobius_add          : out[b, d]     = mobius_addition(x, y, c)       (:27-46)
 *   hm_rows_mobius_scalar_mul   : out[b, d]     = mobius_scalar_mul(r, x, c)     (:49-65, r[b]: one factor per row)
 *   hm_rows_exp_map_zero        : out[b, d]     = exp_map_zero(v, c)             (:68-84)
 *   hm_rows_log_map_zero        : out[b, d]     = log_map_zero(x, c)             (:87-103)
 *   hm_rows_poincare_distance   : out[b]        = distance(x, y, c)              (:106-126)
 *   hm_rows_lorentz_to_poincare : out[b, d]     = lorentz_to_poincare(x[b, d + 1], c)   (:129-140)
 *   hm_rows_poincare_to_lorentz : out[b, d + 1] = poincare_to_lorentz(x[b, d], c)       (:143-163 when standard == 0: as
 *                                 shipped, x0^2 - |x_s|^2 = 1 / (4 c); standard == 1: x0 = (1 + c |x|^2) / (sqrt(c) (1 - c |x|^2)),
 *                                 x_s = 2 x / (1 - c |x|^2), on x0^2 - |x_s|^2 = 1 / c) */
int hm_rows_mobius_add(const float* x_dev, const float* y_dev, int64_t b, int64_t ld, int d, float c, float* out_dev,
                       int64_t ld_out, void* stream);
int hm_rows_mobius_scalar_mul(const float* r_dev, const float* x_dev, int64_t b, int64_t ld, int d, float c,
                              float* out_dev, int64_t ld_out, void* stream);
int hm_rows_exp_map_zero(const float* v_dev, int64_t b, int64_t ld, int d, float c, float* out_dev, int64_t ld_out,
                         void* stream);
int hm_rows_log_map_zero(const float* x_dev, int64_t b, int64_t ld, int d, float c, float* out_dev, int64_t ld_out,
                         void* stream);
int hm_rows_poincare_distance(const float* x_dev, const float* y_dev, int64_t b, int64_t ld, int d, float c,
                              float* out_dev, void* stream);
int hm_rows_lorentz_to_poincare(const float* x_dev, int64_t b, int64_t ld, int d, float c, float* out_dev,
                                int64_t ld_out, void* stream);
int hm_rows_poincare_to_lorentz(const float* x_dev, int64_t b, int64_t ld, int d, float c, int standard, float* out_dev,
                                int64_t ld_out, void* stream);

/* Vector-Jacobian products of the Poincare-ball primitives above (upstream gradient g with leading dimension ld_g, or one
 * value per row for the distance; outputs with leading dimension ld_out).  Only the inputs are read: the row scalars are
 * recomputed.  The derivative is that of the reference's torch expression as torch differentiates it: clamp(n, min = 1e-8)
 * passes the gradient where n >= 1e-8f and gives exactly 0 below, the (n == 0) mask arithmetic of the two zero-maps is
 * walked back term by term, the norm has gradient 0 at the zero vector, atanh' = 1 / (1 - z^2) is infinite at 1 and finite
 * beyond.  No gradient with respect to c.
 *   hm_rows_mobius_add_bwd          : g[b, d]     -> gx, gy        (:27-46)
 *   hm_rows_mobius_scalar_mul_bwd   : g[b, d]     -> gr[b], gx     (:49-65)
 *   hm_rows_exp_map_zero_bwd        : g[b, d]     -> gv            (:68-84)
 *   hm_rows_log_map_zero_bwd        : g[b, d]     -> gx            (:87-103)
 *   hm_rows_poincare_distance_bwd   : g[b]        -> gx, gy        (:106-126)
 *   hm_rows_lorentz_to_poincare_bwd : g[b, d]     -> gx[b, d + 1]  (:129-140)
 *   hm_rows_poincare_to_lorentz_bwd : g[b, d + 1] -> gx[b, d]      (:143-163, or the standard map) */
int hm_rows_mobius_add_bwd(const float* x_dev, const float* y_dev, const float* g_dev, int64_t ld_g, int64_t b, int64_t ld,
                           int d, float c, float* gx_dev, float* gy_dev, int64_t ld_out, void* stream);
int hm_rows_mobius_scalar_mul_bwd(const float* r_dev, const float* x_dev, const float* g_dev, int64_t ld_g, int64_t b,
                                  int64_t ld, int d, float c, float* gr_dev, float* gx_dev, int64_t ld_out, void* stream);
int hm_rows_exp_map_zero_bwd(const float* v_dev, const float* g_dev, int64_t ld_g, int64_t b, int64_t ld, int d, float c,
                             float* gv_dev, int64_t ld_out, void* stream);
int hm_rows_log_map_zero_bwd(const float* x_dev, const float* g_dev, int64_t ld_g, int64_t b, int64_t ld, int d, float c,
                             float* gx_dev, int64_t ld_out, void* stream);
int hm_rows_poincare_distance_bwd(const float* x_dev, const float* y_dev, const float* g_dev, int64_t b, int64_t ld, int d,
                                  float c, float* gx_dev, float* gy_dev, int64_t ld_out, void* stream);
int hm_rows_lorentz_to_poincare_bwd(const float* x_dev, const float* g_dev, int64_t ld_g, int64_t b, int64_t ld, int d,
                                    float c, float* gx_dev, int64_t ld_out, void* stream);
int hm_rows_poincare_to_lorentz_bwd(const float* x_dev, const float* g_dev, int64_t ld_g, int64_t b, int64_t ld, int d,
                                    float c, int standard, float* gx_dev, int64_t ld_out, void* stream);

/* Fused hyperbolic InfoNCE (multimodal/contrastive_loss.py:17-61 of the reference, c = 1): S = -distance / temp between
 * z_text[n, d1] and z_img[n, d1], cross-entropy over rows and over columns against the diagonal, averaged.  The n x n
 * matrix is never stored.  n <= 65536, d1 <= 129.
 *   hm_infonce_fwd : lse_row[n], lse_col[n] (log-sum-exp of the rows / columns of S), diag[n] = S_ii,
 *                    losses[n] = ((lse_row - diag) + (lse_col - diag)) / 2 and *total = their sum in a fixed order
 *   hm_infonce_bwd : gradients of sum_i w[i] * losses[i] with respect to z_text and z_img (either output may be NULL),
 *                    from the two log-sum-exp vectors of the forward call; fixed summation order, no atomics */
int hm_infonce_fwd(const float* zt_dev, const float* zi_dev, int64_t n, int64_t ld_t, int64_t ld_i, int d1, float temp,
                   int sign_mode, float* lse_row_dev, float* lse_col_dev, float* diag_dev, float* losses_dev,
                   float* total_dev, void* stream);
int hm_infonce_bwd(const float* zt_dev, const float* zi_dev, int64_t n, int64_t ld_t, int64_t ld_i, int d1, float temp,
                   int sign_mode, const float* lse_row_dev, const float* lse_col_dev, const float* w_dev,
                   float* g_text_dev, float* g_img_dev, int64_t ld_out, void* stream);
/* Triplet loss (:64-97, c = 1): losses[b] = relu(d(a, p) - d(a, n) + margin) (losses_dev may be NULL); with w_dev the
 * gradients of sum_t w[t] * losses[t] as well (relu' at exactly 0 is 0), without w_dev the forward values alone. */
int hm_triplet_fwd_bwd(const float* a_dev, const float* p_dev, const float* n_dev, int64_t b, int64_t ld, int d1,
                       float margin, int sign_mode, const float* w_dev, float* losses_dev, float* ga_dev, float* gp_dev,
                       float* gn_dev, int64_t ld_out, void* stream);

/* Fused hyperbolic retrieval: one walk over the pair tiles, the n x n distance matrix is never stored.  With
 * D[i, j] = distance(z_text[i], z_img[j]) in the canonical fp32 arithmetic (the bits of hm_batch_distance), c = 1:
 *   rank_t2i[i] = #{ j : D[i, j] < D[i, i] } + #{ j < i : D[i, j] == D[i, i] }
 *   rank_i2t[j] = #{ i : D[i, j] < D[j, j] } + #{ i < j : D[i, j] == D[j, j] }
 * NaN orders as torch.sort orders it (greater than every number, equal to NaN).  Pair i is retrieved at k iff its rank < k.
 * Either output may be NULL.  1 <= n <= 65536, 2 <= d1 <= 129.  No atomics: the same bits on every run.
 * Replaces compute_recall_at_k of the reference (scripts/train_retrieval.py:176-229, called at :403 and :459): B^2 calls of
 * distance(...).item() into a matrix, then torch.topk per row and per column. */
int hm_retrieval_ranks(const float* zt_dev, const float* zi_dev, int64_t n, int64_t ld_t, int64_t ld_i, int d1,
                       int sign_mode, int32_t* rank_t2i_dev, int32_t* rank_i2t_dev, void* stream);
/* Exact k nearest keys of every query: d_out[nq, k], i_out[nq, k] = the k smallest (distance, key index) of each row of
 * hm_batch_distance(q, keys, c), ascending, with the same bits.  NaN distances are never selected; a row with fewer than k
 * selectable keys is padded with (+inf, -1).  exclude_self != 0 skips key i for query i.  d_out doubles as the call's only
 * working memory.  1 <= k <= 128, k <= nk, nq and nk <= 2^20, 2 <= d1 <= 129.
 * Replaces the per-query search of the reference's FAISS branch (index.search(q, k): tokenizer/hyperbolic_merge.py:217,
 * tokenizer/fast_hyperbolic_merge.py:302-304). */
int hm_knn(const float* q_dev, int64_t nq, const float* k_dev, int64_t nk, int64_t ld_q, int64_t ld_k, int d1, float c,
           int sign_mode, int k, int exclude_self, float* d_out_dev, int32_t* i_out_dev, void* stream);
/* Test / tuning hook (results never depend on it): the tile layout hm_retrieval_ranks launches from now on, process-wide.
 * 0 = the default (the faster one of the two), 1 = A and B rows in LDS (the layout of 5.11), 2 = A rows in
 * registers and B rows read as 16-byte LDS broadcasts.  tools/retrieval_probe.py times 1 against 2 in one process. */
int hm_debug_retrieval_layout(int layout);

/* Timing of the last scan launched by hm_pairwise_argmin / hm_pairwise_topk on this engine,
 * measured with HIP events on the stream the kernel ran on (bench.py roofline).
 * *scan_ms = duration of the dominant pair-scan kernel launch(es); *pairs = pairs it covered. */
int hm_last_scan_stats(const hm_engine* e, float* scan_ms, int64_t* pairs, int64_t* emitted, int32_t* passes);

/* Running totals over every pair-scan launch (argmin / top-k modes, not the sampled estimate
 * passes) since engine creation or the last reset: summed event-timed kernel duration, pairs
 * covered and number of launches.  reset != 0 clears the totals after reading. */
int hm_scan_totals(hm_engine* e, double* scan_ms, int64_t* pairs, int64_t* launches, int reset);

/* ---- adjacent-pair histogram of a tokenised corpus (frequency-aware scoring) --------------------------------
 * Exact counts of the adjacent symbol pairs of a corpus, streamed in slabs of lines, with the smallest flat position
 * of every pair (sorting by it gives the order in which the reference's dict first meets the pairs).  Symbols are
 * those of hm_tokenize_batch: in [-(2 + 0x10FFFF), 2^21).  A pair key is ((a + 0x110001) << 22) | (b + 0x110001).
 * Independent of any engine; errors are reported through hm_last_error(NULL).  Every entry point synchronises
 * `stream` before it returns.
 *
 * hm_pairfreq_create / hm_pairfreq_destroy: one counter on device `device`.  initial_capacity (0: 65 536) sizes the
 * first hash tables; a small value is a test hook (the tables grow, and a slab that overflows its table is recounted).
 * Replaces: the dict self.pair_frequencies being filled (frequency_aware_hyperbolic_merge.py:92-112). */
typedef struct hm_pairfreq hm_pairfreq;
int hm_pairfreq_create(hm_pairfreq** out, int device, int64_t initial_capacity);
int hm_pairfreq_destroy(hm_pairfreq* pf);
/* One slab, DEVICE arrays: line l holds sym_dev[offsets_dev[l] .. offsets_dev[l] + len_dev[l]) (len_dev NULL: up to
 * offsets_dev[l + 1]; offsets_dev[0] = 0, n_positions = offsets_dev[n_lines]).  Adds every pair whose two positions lie
 * in one line, at flat position base + p.  LIMITS (HM_E_ARG): n_positions < 2^40, base + n_positions <= 2^62.
 * Replaces: for line in f: tokens = self.tokenize(line.strip()); for pair in zip(tokens, tokens[1:]): ... += 1. */
int hm_pairfreq_add(hm_pairfreq* pf, const int32_t* sym_dev, const int64_t* offsets_dev, const int32_t* len_dev,
                    int64_t n_lines, int64_t n_positions, int64_t base, void* stream);
/* Distinct pairs, total pairs and slab recounts so far (any pointer may be NULL); with the three device arrays (room for
 * out_cap >= n_distinct entries, HM_E_CAPACITY otherwise) also every distinct pair's key, count and first position, in
 * no particular order. */
int hm_pairfreq_read(hm_pairfreq* pf, int64_t* n_distinct, int64_t* n_pairs, int64_t* slab_recounts, uint64_t* keys_dev,
                     uint64_t* counts_dev, int64_t* first_dev, int64_t out_cap, void* stream);

/* ---- character n-gram histogram of a word list (hierarchical tokenizer statistics) --------------------------------
 * Exact counts of every n-gram of length 2..5 of a list of words given as code points (any value: the n-grams are
 * compared code point by code point).  HOST arrays: word w is cps[offsets[w] .. offsets[w + 1]) (offsets[0] = 0,
 * non-decreasing, total below 2^40, fewer than 2^32 words).
 *   HM_NGRAM_WEIGHTED: count(g) = sum over the occurrences of g of weights[w] (int64 >= 0)
 *   HM_NGRAM_DISTINCT: count(g) = number of words that contain g (weights ignored, may be NULL)
 * Independent of any engine; errors are reported through hm_last_error(NULL).  Every entry point synchronises `stream`.
 * initial_capacity (0: 65 536) sizes the first hash table; a small value is a test hook (an overflowing count is redone
 * into larger tables).
 * Replaces: for word in words: for n in range(2, min(6, len(word) + 1)): ... subword_counter[word[i:i+n]] += 1
 * (hierarchical_hyperbolic_merge.py:110-156) and sum(1 for word in self.common_words if token in word) (:193-198). */
#define HM_NGRAM_WEIGHTED 0
#define HM_NGRAM_DISTINCT 1
typedef struct hm_ngram hm_ngram;
int hm_ngram_create(hm_ngram** out, int device, int64_t initial_capacity);
int hm_ngram_destroy(hm_ngram* g);
/* Counts the words; *n_distinct (may be NULL) = distinct n-grams.  Replaces the result of an earlier count. */
int hm_ngram_count(hm_ngram* g, const int32_t* cps, const int64_t* offsets, const int64_t* weights, int64_t n_words, int mode,
                   int64_t* n_distinct, void* stream);
/* The last count's n-grams into HOST arrays (room for out_cap >= n_distinct, HM_E_CAPACITY otherwise; all three or none):
 * n-gram k is cps[pos[k] .. pos[k] + len[k]) of the last count's input, with its count; no particular order.
 * *recounts (may be NULL): counts redone into larger tables since creation. */
int hm_ngram_read(hm_ngram* g, int64_t* pos, int32_t* len, int64_t* counts, int64_t out_cap, int64_t* recounts, void* stream);

/* ---- per-class running minima of the pair distance (hierarchical tokenizer step selection) -------------------------
 * Every live row carries a code in [0, HM_CM_CODES); a pair i < j belongs to the class of its unordered code pair,
 * cls(a, b) = lo * HM_CM_CODES - lo * (lo - 1) / 2 + (hi - lo) with lo = min(a, b), hi = max(a, b).  A record is
 * uint32[4] {found, bits(d), i, j}: the lexicographic minimum of (bits(d), i, j) over the class's pairs, d the engine's
 * canonical distance (the one hm_pairwise_candidates lists), NaN excluded, NO threshold.  found = 0: the class is empty.
 * One handle per engine, on the engine's device; errors through hm_last_error(engine).  Every entry point synchronises.
 * Replaces: min over the candidate list of hierarchical_hyperbolic_merge.py:279-428, filtered per phase. */
#define HM_CM_CODES 10
#define HM_CM_CLASSES 55
#define HM_CM_SLOTS 57
typedef struct hm_classmin hm_classmin;
int hm_classmin_create(hm_classmin** out, hm_engine* e);
int hm_classmin_destroy(hm_classmin* cm);
/* HOST codes[r - row_begin] of rows [row_begin, row_end) (each < HM_CM_CODES). */
int hm_classmin_set_codes(hm_classmin* cm, const uint8_t* codes, int64_t row_begin, int64_t row_end, void* stream);
/* One exact pass over every pair of the live rows: out[4 * q ..] = record of class q, q < HM_CM_CLASSES (HOST). */
int hm_classmin_build(hm_classmin* cm, float c, uint32_t* out, void* stream);
/* Row `row` against rows [0, row): out[4 * q ..] (q < HM_CM_CLASSES) = record of class q over the pairs (i, row); and over the
 * HOST list partners[] (index | 1 << 28: exception list A, | 1 << 29: exception list B; every index below `row`):
 * out[4 * HM_CM_CLASSES ..] = record of the A pairs, out[4 * (HM_CM_CLASSES + 1) ..] = record of the B pairs. */
int hm_classmin_fold(hm_classmin* cm, int64_t row, float c, const int32_t* partners, int64_t n_partners, uint32_t* out,
                     void* stream);

/* ---- shortest-path lengths and connected components of an undirected graph (hierarchy-distortion evaluation) --------
 * The graph is a symmetric CSR built by the caller: HOST row_ptr int64[n + 1] (row_ptr[0] = 0, non-decreasing) and col
 * int32[nnz], 1 <= n <= 2^24, nnz < 2^31, every index in [0, n) (HM_E_ARG otherwise).  Self-loops and repeated entries are
 * harmless, a node of degree 0 is legal.  Independent of any engine; errors through the global last-error message; every
 * entry point synchronises `stream`.  Path lengths come from a bit-parallel multi-source BFS: the distinct sources of a
 * call own one bit each, a node carries W 64-bit words of seen / frontier / next, and a call whose sources exceed 64 * W
 * runs several passes; W is the largest value with 3 * n * W * 8 bytes <= 1 GiB (at least 1), and the default knob
 * "graph_pass_words" lowers it (tests); "graph_chunk_levels" is the number of BFS levels enqueued between two reads of the
 * device-side counters (16).
 * Replaces: nx.shortest_path_length(graph, a, b) once per sampled pair (scripts/eval_hierarchy.py:125-136). */
typedef struct hm_graph hm_graph;
int hm_graph_create(hm_graph** out, int device);
int hm_graph_destroy(hm_graph* g);
int hm_graph_set_csr(hm_graph* g, const int64_t* row_ptr, const int32_t* col, int64_t n, void* stream);
/* labels_dev int32[n]: the smallest node index of the node's component; *n_components (HOST, may be NULL). */
int hm_graph_components(hm_graph* g, int32_t* labels_dev, int64_t* n_components, void* stream);
/* HOST src[p], dst[p] -> out_dev int32[n_pairs]: edges on a shortest path, 0 where src == dst, -1 where there is none. */
int hm_graph_pair_lengths(hm_graph* g, const int32_t* src, const int32_t* dst, int64_t n_pairs, int32_t* out_dev, void* stream);
/* HOST src[n_src] and cols[n_cols] (cols NULL: every node, n_cols ignored) -> out_dev int16[n_src, ld]: out[s, m] = length
 * from src[s] to cols[m], -1 where there is none.  HM_E_CAPACITY when a listed node lies more than 32767 edges away. */
int hm_graph_distance_rows(hm_graph* g, const int32_t* src, int64_t n_src, const int32_t* cols, int64_t n_cols, int16_t* out_dev,
                           int64_t ld, void* stream);
/* Of the last call above: BFS levels (component iterations) that did work, kernel launches enqueued, passes, words per
 * node (any pointer may be NULL). */
int hm_graph_last_stats(const hm_graph* g, int64_t* levels, int64_t* launches, int64_t* passes, int64_t* words);

/* ---- Riemannian optimiser steps for rows on the unit hyperboloid -----------------------------------
 * One fused, in-place step per call: x [table_rows, ld_x] holds points with <x, x> = -1 under <a, b> = -a0 b0 + sum ak bk
 * (d1 = d + 1 columns, 2 <= d1 <= 129), g the Euclidean gradient of a loss with respect to them, m the first moment
 * (tangent at x, transported to the new point), v (RAdam) one second moment per row.  Curvature only scales distances
 * and is folded into lr by the caller.
 *   dense   (rows_dev NULL, n == table_rows): row t of g updates row t of x, m, v;
 *   indexed (rows_dev int64[n] on the device): row t of the compact g [n, ld_g] updates row rows_dev[t] of x, m, v; an
 *           index outside [0, table_rows) is skipped (nothing is written for it), indices must be distinct.
 * hm_rsgd_step:  m+ = momentum m + (1 - dampening) u, step along m+ (nesterov: u + momentum m+); with momentum == 0
 *                m_dev must be NULL, dampening is ignored and the step is along u.
 * hm_radam_step: m+ = beta1 m + (1 - beta1) u, v+ = beta2 v + (1 - beta2) <u, u>, step along (m+ / bc1) / (sqrt(v+ / bc2) + eps);
 *                bc1 = 1 - beta1^t and bc2 = 1 - beta2^t come from the caller (nothing is read back from the device).
 * Engine-independent; errors through hm_last_error(NULL); asynchronous on `stream`.  HM_E_ARG before the device is touched
 * for a NULL required pointer, d1 outside 2..129, a leading dimension below d1, n < 0 (or != table_rows in the dense
 * form), lr negative or not finite, momentum / dampening / beta outside [0, 1), bc <= 0, eps < 0.  n == 0: HM_OK, no launch.
 * Replaces: nothing the reference runs -- its riemannian_gradient / exp_map / parallel_transport (lorentz_model.py) are
 * never called and do not compose into a step that stays on the hyperboloid. */
int hm_rsgd_step(float* x_dev, int64_t ld_x, const float* g_dev, int64_t ld_g, float* m_dev, int64_t ld_m, const int64_t* rows_dev,
                 int64_t n, int64_t table_rows, int d1, float lr, float momentum, float dampening, int nesterov, void* stream);
int hm_radam_step(float* x_dev, int64_t ld_x, const float* g_dev, int64_t ld_g, float* m_dev, int64_t ld_m, float* v_dev,
                  const int64_t* rows_dev, int64_t n, int64_t table_rows, int d1, float lr, float beta1, float beta2, float eps,
                  float bc1, float bc2, void* stream);

/* ---- graph embedding: the edge-softmax loss on a Lorentz table and its negative sampler ---------------
 * x [table_rows, ld] fp32 points of the hyperboloid (d1 = d + 1 columns, 2 <= d1 <= 129), index int64 [n, 2 + k] on the
 * device: column 0 the anchor, column 1 the positive, columns 2.. the negatives.  A negative outside [0, table_rows) is a
 * skipped slot (-1 is the documented mask), a sample whose anchor or positive lies outside is skipped whole (loss 0);
 * neither is dereferenced.  With u_j = x_u0 x_j0 - sum_s x_us x_js in the canonical order (exactly 1 for a partner that is
 * the anchor itself) and d_j = acosh(max(u_j, 1)) / sqrt(c) -- the bits of hm_rows_distance under HM_SIGN_LORENTZ --
 *   loss[b] = d_0 + log sum_{j live} exp(-d_j)                        (positive inside the sum, shifted by its maximum)
 *   a_j     = ([j = 0] - softmax(-d)_j) / (sqrt(c) sqrt(u_j^2 - 1)), and 0 where u_j <= 1 (NOT the infinite derivative of
 *             hm_rows_distance_bwd at coincident rows).
 * hm_edge_loss_fwd writes loss_dev [n] and weights_dev [n, 1 + k] = a_j (0 for a skipped slot), the only state between
 * the two calls.  hm_edge_loss_bwd takes grad_loss_dev [n] and writes the Euclidean gradient in COO form, slot order:
 * values_dev [n * (2 + k), d1], row (b, 0) = g_b sum_j a_j (x_j0, -x_js), row (b, 1 + j) = g_b a_j (x_u0, -x_us), and
 * coo_dev int64 [n * (2 + k)] = index with a skipped slot replaced by the anchor (by 0 when the sample is skipped), its
 * value row zero.  Every row is written once, no atomics: two calls on the same inputs give the same bits.
 * Engine-independent; errors through hm_last_error(NULL); asynchronous on `stream`.  HM_E_ARG before the device is touched
 * for a NULL pointer, d1 outside 2..129, ld < d1, negative table_rows / n / k, c not positive and finite.  n == 0: HM_OK,
 * no launch.  Replaces: nothing the reference runs (it has no trainer). */
int hm_edge_loss_fwd(const float* x_dev, int64_t ld, int64_t table_rows, int d1, const int64_t* index_dev, int64_t n, int64_t k,
                     float c, float* loss_dev, float* weights_dev, void* stream);
int hm_edge_loss_bwd(const float* x_dev, int64_t ld, int64_t table_rows, int d1, const int64_t* index_dev, int64_t n, int64_t k,
                     float c, const float* weights_dev, const float* grad_loss_dev, float* values_dev, int64_t* coo_dev, void* stream);
/* Test / tuning hook: the work decomposition of the two calls above from now on -- 0: one lane group per sample, 1: one wave
 * per sample (the default).  Losses and gradients agree to rounding (another order of the sums over the
 * partners); d_0 and every u_k are the same bits. */
int hm_debug_edge_loss_form(int form);

/* ---- entailment cones: a directed hierarchy loss on a Lorentz table ------------------------------------------
 * The hyperbolic entailment cones of Ganea, Becigneul & Hofmann (ICML 2018) on points of the unit hyperboloid.  x, index and
 * the rules for indices outside [0, table_rows) are those of hm_edge_loss_fwd: column 0 the anchor, column 1 the positive,
 * columns 2.. the negatives; a skipped slot and a skipped sample are never dereferenced.  Of a slot's two rows one is the apex
 * a (the parent), the other the child b: apex_role 0 makes the anchor the apex of every slot (the negatives are corrupted
 * children), apex_role 1 every partner (the anchor is the child, the negatives corrupted parents).  With
 *   u = a0 b0 - sum_s a_s b_s and n = sqrt(sum_s a_s^2) in the canonical order,  w = sqrt(u^2 - 1),  A = (b0 - a0 u) / (n w),
 *   ext = acos(clamp(A, +-(1 - 2^-20))),  aper = asin(min(2 aperture_k / n, 1 - 2^-10)),  m = ext - aper,  E = max(0, m):
 *   loss[b] = E_0 + sum_{j >= 1 live} max(0, margin - E_j).
 * A partner that is the anchor itself (same index), a slot with u <= 1 and an apex at the origin (n = 0) are flat: E = 0 and
 * no gradient; a clamped factor is a constant (at d1 = 2, a line, every A is +-1 and counts as clamped); a negative inside
 * the cone (m <= 0) contributes margin and no gradient.
 * Angles do not depend on curvature: there is no c.
 * hm_cone_loss_fwd writes loss_dev [n] and weights_dev [n, 1 + k, 4] (16-byte aligned), per slot the hinge-scaled
 * coefficients (alpha, the anchor's e0 factor, nu / n, the partner's e0 factor) of DESIGN.md 5.21, zero for a skipped or
 * inactive slot: the only state between the two calls.  hm_cone_loss_bwd takes grad_loss_dev [n] and writes the Euclidean
 * gradient in COO form exactly as hm_edge_loss_bwd does: values_dev [n * (2 + k), d1], coo_dev int64 [n * (2 + k)] = index
 * with a skipped slot replaced by the anchor (by 0 when the sample is skipped), its value row zero.  Every row is written
 * once, no atomics: two calls on the same inputs give the same bits.
 * Engine-independent; errors through hm_last_error(NULL); asynchronous on `stream`.  HM_E_ARG before the device is touched
 * for a NULL pointer, a misaligned weights_dev, d1 outside 2..129, ld < d1, negative table_rows / n / k, aperture_k not
 * positive and finite, margin negative or not finite, apex_role other than 0 or 1.  n == 0: HM_OK, no launch.
 * Replaces: nothing the reference runs (it has no trainer and no directed objective). */
int hm_cone_loss_fwd(const float* x_dev, int64_t ld, int64_t table_rows, int d1, const int64_t* index_dev, int64_t n, int64_t k,
                     float aperture_k, float margin, int apex_role, float* loss_dev, float* weights_dev, void* stream);
int hm_cone_loss_bwd(const float* x_dev, int64_t ld, int64_t table_rows, int d1, const int64_t* index_dev, int64_t n, int64_t k,
                     float aperture_k, float margin, int apex_role, const float* weights_dev, const float* grad_loss_dev,
                     float* values_dev, int64_t* coo_dev, void* stream);
/* Test / tuning hook: the work decomposition of the two calls above from now on -- 0: one lane group per sample, 1: one wave
 * per sample (the default).  Losses and anchor rows agree to rounding (another order of the sums over the
 * partners); every slot's coefficients and partner rows are the same bits.  Replaces: nothing the reference runs. */
int hm_debug_cone_loss_form(int form);

/* ---- Lorentz-centroid pooling of token rows ---------------------------------------------------------------
 * Serves embedding.pooling.lorentz_centroid / HyperbolicEmbeddingBag and HyperbolicTokenizer.embed_batch: one point of the
 * hyperboloid per line from the rows of its tokens (Law et al., ICML 2019).  x [table_rows, ld] fp32 points of the unit
 * hyperboloid (d1 columns, 2 <= d1 <= 129), ids int64 [t], offsets int64 [n + 1] non-decreasing within [0, t] (clamped into
 * it otherwise), lengths int32 [n] or NULL (clamped to the span), weights fp32 [t] or NULL, all on the device.  Segment i is
 * ids[offsets[i] : offsets[i] + len_i]; a token is live when it lies inside that length and its id lies in [0, table_rows)
 * (-1 is the documented padding); nothing else is dereferenced.
 *   s_i = sum_t w_t x_{ids[t]},  q_i = s_i0^2 - |s_is|^2,  mu_i = s_i / sqrt(q_i);  without a live token, or where q_i is not
 *   positive and finite, mu_i = (1, 0, .., 0) and the segment's gradient is zero.
 * hm_centroid_fwd writes mu_dev [n, d1] and inv_nu_dev [n] = 1 / sqrt(q_i) (0 for a degenerate segment), the only state
 * between the two calls.  hm_centroid_bwd takes grad_dev [n, d1] and, with h_i = (g_i + (g_i . mu_i) J mu_i) / sqrt(q_i),
 * J = diag(-1, 1, .., 1), writes the Euclidean gradient in COO form, position order: values_dev [t, d1] row p = w_p h_i and
 * coo_dev int64 [t] = ids[p]; a skipped position (slack behind a length, id out of range, outside every span) has index 0 and
 * a zero row.  grad_weights_dev [t] (or NULL: then no table row is read) receives h_i . x_{ids[p]}, 0 where skipped.  Every
 * row is written once, no atomics: two calls on the same inputs give the same bits.  Engine-independent; errors through
 * hm_last_error(NULL); asynchronous on `stream`.  HM_E_ARG before the device is touched for a NULL table, d1 outside 2..129,
 * ld < d1, negative table_rows / t / n, NULL offsets with n > 0, NULL ids with t > 0.  n == 0: the forward launches nothing,
 * the backward zero-fills its outputs.  Replaces: nothing the reference runs (it has no pooling). */
int hm_centroid_fwd(const float* x_dev, int64_t ld, int64_t table_rows, int d1, const int64_t* ids_dev, int64_t t,
                    const int64_t* offsets_dev, const int32_t* lengths_dev, const float* weights_dev, int64_t n, float* mu_dev,
                    float* inv_nu_dev, void* stream);
int hm_centroid_bwd(const float* x_dev, int64_t ld, int64_t table_rows, int d1, const int64_t* ids_dev, int64_t t,
                    const int64_t* offsets_dev, const int32_t* lengths_dev, const float* weights_dev, int64_t n, const float* mu_dev,
                    const float* inv_nu_dev, const float* grad_dev, float* values_dev, int64_t* coo_dev, float* grad_weights_dev,
                    void* stream);
/* Test / tuning hook: the work decomposition of the two calls above from now on -- 0: one lane group per segment, 1: one wave
 * per segment, -1: chosen per call from n and the mean segment length (the default).  Results agree to
 * rounding (another order of the sum over the tokens of a segment). */
int hm_debug_centroid_form(int form);

/* Negative sampler.  The graph is a symmetric CSR as for hm_graph_set_csr (HOST arrays, 1 <= n < 2^31) whose rows are
 * additionally sorted and free of repeats (HM_E_ARG otherwise; hm_negsample_check_csr is that check alone and touches no
 * device).  hm_negsample_sample: pairs_dev int64 [n_pairs, 2] -> out_dev int64 [n_pairs, 2 + k], columns 0 and 1 copied,
 * slot j of sample b the first candidate of attempts t = 0 .. max_tries - 1 that is neither the anchor nor adjacent to it,
 * candidate = (uint64(r) * n) >> 32 with r the first output word of Philox4x32-10 under key (seed low, seed high) and
 * counter (b, j, t, step); -1 when every attempt was rejected or the anchor lies outside [0, n).  0 <= step < 2^32,
 * 1 <= max_tries <= 65536.  Asynchronous on `stream`; hm_negsample_set_csr synchronises it. */
typedef struct hm_negsample hm_negsample;
int hm_negsample_create(hm_negsample** out, int device);
int hm_negsample_destroy(hm_negsample* g);
int hm_negsample_check_csr(const int64_t* row_ptr, const int32_t* col, int64_t n);
int hm_negsample_set_csr(hm_negsample* g, const int64_t* row_ptr, const int32_t* col, int64_t n, void* stream);
int hm_negsample_sample(hm_negsample* g, const int64_t* pairs_dev, int64_t n_pairs, int64_t k, uint64_t seed, int64_t step,
                        int max_tries, int64_t* out_dev, void* stream);

/* Graph reconstruction: where the graph neighbours of a node land when every other node is ranked by its
 * distance to it, as integer counts, without a [nodes, V] distance slab.  x_dev is fp32 [V, d1] with leading dimension ld;
 * D[u, v] is the canonical fp32 distance at c = 1 under the "lorentz" sign (the bits of hm_batch_distance).  The calls take no
 * curvature: a division by sqrt(c) could merge distinct fp32 distances into ties.  The graph is a CSR without self-loops whose
 * rows are sorted and free of repeats (what hm_negsample_check_csr accepts), symmetric or not.  A slot is a directed edge
 * e = (u, o), o in N(u); slots with the same anchor are contiguous and form a segment.  Per slot, int32:
 *   less_all[e]  = #{ v != u    : D[u, v] <  D[u, o] }
 *   equal_all[e] = #{ v != u    : D[u, v] == D[u, o] }      (>= 1: v = o)
 *   less_nb[e]   = #{ v in N(u) : D[u, v] <  D[u, o] }
 *   equal_nb[e]  = #{ v in N(u) : D[u, v] == D[u, o] }      (>= 1)
 * NaN orders as in hm_retrieval_ranks: greater than every number, equal to NaN; a NaN pivot has less = the number of
 * distances that are numbers and equal = the number of NaN ones.  From the counts
 *   rank[e]      = 1 + less_all[e] - less_nb[e]             (position among the non-neighbours, ties optimistic)
 *   precision[e] = (less_nb[e] + equal_nb[e]) / (less_all[e] + equal_all[e])
 *   mean rank    = sum_e rank[e] / #slots;   AP(u) = mean of precision over the slots of u;   mAP = mean of AP(u), deg(u) > 0.
 * hm_recon_slots lists the slots of n_seg anchors in CSR order: nodes_dev int64 [n_seg] (NULL: node g is anchor g, n_seg = V),
 * seg_ptr_dev int64 [n_seg + 1] the running sum of their degrees from 0, n_slots = seg_ptr[n_seg]; it writes slot_anchor,
 * slot_pivot and slot_seg (the position of the slot's anchor in nodes), int32 [n_slots] each.
 * hm_recon_counts takes such slots (any list of contiguous segments will do: slot e belongs to segment slot_seg[e], which
 * spans the slots seg_ptr[g] .. seg_ptr[g + 1] - 1) and writes the four vectors; u_scratch_dev fp32 [n_slots] is its only
 * working memory (the clamped argument of acosh of every slot's pivot).  A slot whose anchor or pivot lies outside [0, V), or
 * whose segment outside [0, n_seg), is never dereferenced and gets -1 in all four vectors; the neighbour counts of the other
 * slots of its segment are then unspecified.  Every element is written once, no atomics: two calls give the same bits.
 * Engine-independent; errors through hm_last_error(NULL); asynchronous on `stream`.  HM_E_ARG before the device is touched for
 * a NULL pointer (with n_slots == 0 only x_dev / row_ptr_dev and seg_ptr_dev are required), d1 outside 2..129, ld < d1,
 * V outside 1..2^31 - 1, negative (or >= 2^31) nnz, n_seg, n_slots, slots without a segment.  n_slots == 0 launches nothing.
 * Replaces: nothing the reference runs (it never evaluates an embedding against its graph). */
int hm_recon_slots(const int64_t* row_ptr_dev, const int32_t* col_dev, int64_t V, int64_t nnz, const int64_t* nodes_dev,
                   int64_t n_seg, const int64_t* seg_ptr_dev, int64_t n_slots, int32_t* slot_anchor_dev, int32_t* slot_pivot_dev,
                   int32_t* slot_seg_dev, void* stream);
int hm_recon_counts(const float* x_dev, int64_t ld, int64_t V, int d1, const int32_t* slot_anchor_dev, const int32_t* slot_pivot_dev,
                    const int32_t* slot_seg_dev, const int64_t* seg_ptr_dev, int64_t n_slots, int64_t n_seg, int32_t* less_all_dev,
                    int32_t* equal_all_dev, int32_t* less_nb_dev, int32_t* equal_nb_dev, float* u_scratch_dev, void* stream);
/* Test / tuning hook (results never depend on it): the tile layout of hm_recon_counts' walk from now on, process-wide.
 * 0 = the default (chosen by width from measurements: layout 1 for d1 < 97, layout 2 from there on), 1 = anchor
 * and partner rows in LDS, 2 = anchor rows in registers and partner rows read as 16-byte LDS broadcasts (d1 >= 9; narrower
 * rows always take layout 1). */
int hm_debug_recon_layout(int layout);

/* Gromov delta-hyperbolicity: how far a metric is from a tree's, per base point, as one fused walk over the
 * (max, min) semiring without a Gromov-product matrix.  d_dev is a row-major [n, n] distance matrix with leading dimension ld,
 * of which only the upper triangle is read: D(i, j) := d[min(i, j), max(i, j)]; the diagonal is read as it is given.
 * base_dev int32 [n_base] holds positions w in 0..n-1; per base the call writes one value and one witness (i, j, k), int32
 * [n_base, 3].
 *   hm_gromov_delta_i16 (int16 distances):  B_w(i, j) = D(i, w) + D(j, w) - D(i, j), twice the Gromov product, an integer.
 *     Precondition: 0 <= d <= 32767 and the triangle inequality holds, so 0 <= B <= 65534 fits 16 unsigned bits.
 *     value (int32) = 2 delta_w = max_{i <= j} [ max_k min(B(i, k), B(k, j)) - B(i, j) ].
 *   hm_gromov_delta_f32 (float distances):  A_w(i, j) = 0.5f * ((D(i, w) + D(j, w)) - D(i, j)) + 0.0f, evaluated in exactly
 *     this order without contraction (the + 0.0f stores -0 as +0).  Precondition: every entry is finite.
 *     value (float) = delta_w = max_{i <= j} fl( max_k min(A(i, k), A(k, j)) - A(i, j) ); max and min are exact, so the value
 *     has the bits of a float32 restatement in numpy.
 * Witness: among the maximising pairs the smallest i, then the smallest j >= i, then the smallest k that attains the inner
 * maximum of that pair.  The maximum of delta_w over all w is the four-point delta; a tree metric gives 0.
 * A base outside [0, n) is never dereferenced: value -1, witness (-1, -1, -1).  With a precondition violated the values are
 * unspecified, but no index is ever derived from matrix data, so such a call cannot read out of bounds.
 * workspace: hm_gromov_workspace_bytes(n, n_base) bytes of device memory = 16 bytes per base and 128 x 128 tile of the upper
 * triangle (one record per block; -1 for sizes the calls refuse), not initialised by the caller, free for reuse once the call
 * has run.  Every output is written once by one thread, no atomics: two calls give the same bytes.
 * Engine-independent; errors through hm_last_error(NULL); asynchronous on `stream`.  HM_E_ARG before the device is touched for
 * a NULL pointer, n outside 1..32768, ld < n, n_base < 0 or n_base > n.  n_base == 0 launches nothing and returns HM_OK.
 * Replaces: nothing the reference runs (its AdaptiveCurvatureTokenizer, the one place that would choose a curvature, cannot
 * be run: SURVEY F8). */
int hm_gromov_delta_i16(const int16_t* d_dev, int64_t n, int64_t ld, const int32_t* base_dev, int64_t n_base, int32_t* value_out_dev,
                        int32_t* witness_out_dev, void* workspace, void* stream);
int hm_gromov_delta_f32(const float* d_dev, int64_t n, int64_t ld, const int32_t* base_dev, int64_t n_base, float* value_out_dev,
                        int32_t* witness_out_dev, void* workspace, void* stream);
int64_t hm_gromov_workspace_bytes(int64_t n, int64_t n_base);
/* Test / tuning hook (results never depend on it while the preconditions hold): the path of hm_gromov_delta_i16 from now on,
 * process-wide.  0 = the default (the packed path, chosen by measurement: DESIGN.md 5.20), 1 = 32-bit integer min / max, one
 * output per lane (the path hm_gromov_delta_f32 always takes, on order-preserving keys), 2 = packed 16-bit min / max, two
 * outputs per lane. */
int hm_debug_gromov_form(int form);

/* Test hook: pretend the previous refresh ended on this emission cut (bits of u'); the next whole-table top-k
 * search starts from it as given and has to notice by itself when it is too tight. */
int hm_debug_force_cut(hm_engine* e, uint32_t cut_bits, int64_t k, float c);

/* Test / tuning hook for the pair scan's work decomposition (results never depend on it): "big_rows" (512-row blocks for
 * launches covering at least the pairs of this many rows), "chunk", "tail", "tail_div", "shape", "incr_topk", "phases" / "ph_share0..4" / "ph_div1..5" (item list of the scan), "dyn" (0: one block per item instead of the resident grid
 * that draws its items from a device counter) and "dyn_slots" (size of that resident grid; 0 = what the device holds), "head" (k-steps of the argmin scan's
 * head test: the value the library was built with, 3, or 0 for the kernels without the test; the library launches the head kernels
 * only where it expects a tight bound -- from the third merge into a table on), "head_force" (1: on every eligible launch), "head_ring" (the head kernels' partner-tile
 * ring: 1 = 64-column padded slots, three in flight; 2 = 64-column slots of the tile's own size, four in flight; 0 = the 128-column
 * ring of every other kernel), "head_blocks" (3 (default) = the head kernels' ring 3: four 64-column slots of the tile's own size and nothing
 * behind them, three blocks per CU and three waves per SIMD -- span 2 at 8 and 13 chunks, ring 1 otherwise; 2 = ring 1), "head_span" (ring slots a head kernel computes between two barriers: 2 (default) = 128 columns as one
 * pipeline with a straight-line body for the tiles right of the block's rows, or 1; rings 1 and 2 only, and span 1 where a width's ring has fewer
 * than four slots), "pipeline" (0: the standard loop
 * strictly sequential), "pipeline_pairs", "pipe_fault_at", "exact_search" (1: every top-k / count through the prefilter-free
 * exact path that is otherwise the last resort of a search whose survivors fit no emission cut), "kc_even" (default knob only:
 * bf16 image rows padded to whole 16-slot k-steps), and the two default knobs of the graph component above.  hm_debug_set_default_knob applies to every
 * engine created afterwards in this process (clear != 0 removes the default `name`, or all of them when name is NULL / "").
 * The shipped library reads no environment variable for these; tuning builds (-DHM_TUNING) also accept HM_TUNE_<NAME>. */
int hm_debug_set_knob(hm_engine* e, const char* name, double value);
int hm_debug_set_default_knob(const char* name, double value, int clear);

#ifdef __cplusplus
}
#endif
#endif /* HYPMERGE_H */
