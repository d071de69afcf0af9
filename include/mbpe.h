/*
 * mbpe.h -- C-ABI of the MI355X-native BPE trainer hot path.
 *
 * Drop-in boundary for justinhj/minbpe-cc's training path (both tie-breaks), its encode and its decode.
 * The reference has no FFI layer of its own; every entry point
 * below names the reference code it replaces (paths relative to the
 * reference checkout, code/include/...).  INTEGRATION.md shows the binding a
 * reference maintainer would add inside Tokenizer::train.
 *
 * Conventions
 *   - plain pointers and sizes only; no C++ or torch types cross the boundary
 *   - every function returns 0 (MBPE_OK) or a negative mbpe_status; the text
 *     of the last error of the calling thread is mbpe_last_error()
 *   - the caller owns every buffer it passes; the context owns device memory
 *   - one context per GPU and per thread (thread-compatible, like the
 *     reference's Tokenizer, which is not thread-safe: Tokenizer.h:67-72)
 *   - there is NO CPU fallback: without a usable HIP device mbpe_create fails
 *
 * Token ids: the reference's Token is a uint32_t (Tokenizer.h:37-38).  The device stream holds
 * 16-bit slots while the ids allow it: up to MBPE_MAX_VOCAB_BASIC for a single-chunk corpus and
 * MBPE_MAX_VOCAB_CHUNKED when chunk boundaries are present (up to MBPE_MAX_VOCAB_ENDBIT a chunked
 * stream marks "last token of its chunk" with one slot bit; beyond that it keeps a barrier slot
 * after every chunk instead: one more slot per chunk, ids use all 16 bits).  A larger vocab_size
 * (up to MBPE_MAX_VOCAB_WIDE) trains its first merges on the slot stream and the rest on 32-bit
 * tokens with 64-bit pair keys (csrc/wide.h: one merge per pass, one GPU).  With the `first`
 * tie-break it does so only when the option "first_wide" is 1 (Tokenizer::train, the CLI and
 * mbpe_tok_train set it); otherwise, and with several ranks, such a request returns MBPE_ERR_VOCAB.
 */
#ifndef MBPE_H
#define MBPE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MBPE_API __attribute__((visibility("default")))

#define MBPE_MAX_VOCAB_BASIC   65534u
#define MBPE_MAX_VOCAB_ENDBIT  32766u
#define MBPE_MAX_VOCAB_CHUNKED 65518u
#define MBPE_MAX_VOCAB_WIDE    16777216u   /* 2^24: the 32-bit continuation */
#define MBPE_NO_BARRIER 0xFFFFFFFFu

typedef enum {
    MBPE_NEED_EXCHANGE =  1,  /* external-transport mode only: reduce the exchange buffer, then
                                 call mbpe_comm_exchange_done */
    MBPE_OK            =  0,
    MBPE_ERR_ARG       = -1,  /* bad argument (NULL, vocab_size < 256: Tokenizer.h:492) */
    MBPE_ERR_NO_DEVICE = -2,  /* no HIP device / extension unusable */
    MBPE_ERR_HIP       = -3,  /* a HIP runtime call failed */
    MBPE_ERR_VOCAB     = -4,  /* vocab_size beyond MBPE_MAX_VOCAB_WIDE, or beyond the 16-bit slot format where the
                                 32-bit continuation does not apply (several ranks; `first` tie-break without the
                                 option "first_wide") */
    MBPE_ERR_STATE     = -5,  /* call order violated (e.g. steps before begin) */
    MBPE_ERR_OOM       = -6,  /* device or host allocation failed */
    MBPE_ERR_REGEX     = -7,  /* PCRE2 unavailable, compile or match error */
    MBPE_ERR_SPLIT_GAP = -8,  /* mbpe_splitter_split: PCRE2 left bytes of a host span in no match (invalid UTF-8); use
                                 mbpe_presplit, which skips such bytes like the reference does */
    MBPE_ERR_COMM      = -9,  /* RCCL unavailable or a collective failed */
    MBPE_ERR_OVERFLOW  = -10, /* pair table or count overflow detected on device */
    MBPE_ERR_IO        = -11  /* file could not be read / written */
} mbpe_status;

typedef struct mbpe_ctx mbpe_ctx;

/* Per-run statistics; all times are milliseconds of device time measured
 * with HIP events on the context's stream. */
typedef struct {
    uint64_t n_bytes;          /* corpus bytes loaded */
    uint64_t n_chunks;         /* chunks after dropping NUL-quirk chunks */
    uint64_t n_slots;          /* physical stream slots right now */
    uint64_t n_live;           /* live tokens right now */
    uint32_t n_merges;         /* merges performed so far */
    uint32_t n_compactions;    /* stream compactions performed */
    uint64_t n_pairs;          /* members of the device's pair table (what mbpe_get_pairs returns): PairCount::get_count
                                  less those of the transient zero-count pairs (X,a), which the reference inserts between
                                  two touching matches, that the device never inserted ("Exactness of the
                                  parallel merge") */
    float    ms_pair_count;    /* last pair-count scan kernel */
    float    ms_begin;         /* widen + table build + first argmax */
    float    ms_steps;         /* all merge steps so far */
    uint32_t pair_count_launches;
    uint32_t merge_launches;   /* merge-kernel launches timed: grows only while the option "time_kernels" is 1, by one per
                                  stream pass that merged something, and accumulates over the trainings of a loaded corpus
                                  (mbpe_load_corpus* resets it, mbpe_train_begin does not); so do ms_merge_kernel and
                                  the fused_* fields below */
    float    ms_merge_kernel;  /* summed duration of those launches */
    uint32_t n_batches;        /* stream passes that merged something (several merges can share one) */
    uint32_t n_fused;          /* of them: fused passes (large batches, merged stream written to the other buffer) */
    uint32_t n_fused_dropped;  /* fused passes whose output was abandoned because validation kept only a prefix */
    uint32_t cut_conflict;     /* batches ended by a pair that depends on an earlier pair of the batch */
    uint32_t cut_bucket;       /* ... by a full lookup bucket */
    uint32_t cut_single;       /* ... by a zero-count pair or a (t,t) pair that is merged alone: every (t,t) pair under
                                  the bound-walking selection ("threshold_select" 0, or as the fallback); under the
                                  threshold selection only one that finds no stand-in id left in its batch */
    uint32_t cut_full;         /* batches that reached the size limit */
    uint32_t n_validation_drops; /* pairs selected but not merged in that pass (validation) */
    float    ms_grow_table;    /* host wall time spent growing the pair table (allocation + rehash) */
    float    ms_compact;       /* host wall time spent compacting the stream */
    uint32_t n_table_grows;
    uint32_t n_sel_fallback;   /* batches chosen by the bound-walking selection instead of the threshold gather */
    uint32_t fused_launches;   /* fused passes timed ("time_kernels" 1 only; accumulates like merge_launches): one per
                                  sequence that n_fused counts, abandoned ones included */
    float    ms_fused_kernel;  /* their summed duration */
    uint64_t fused_slots;      /* stream slots those passes read (and wrote): n_slots at each pass, summed */
    uint32_t n_sel_retry;      /* batches whose first candidate gather overflowed (threshold found among the block bounds) */
    uint32_t adapt_limit;      /* current batch size limit learnt from validation */
    uint64_t n_sel_blocks;     /* 1024-entry blocks of the pair table read by the candidate gathers */
    uint32_t size_hist[8];     /* passes by merges committed: 1, 2-3, 4-7, 8-15, 16-31, 32-63, 64-127, 128 and more */
    uint32_t n_skipped;        /* dependent candidates passed over by the selection (merged in a later pass) */
    uint32_t n_skip_cut;       /* ... that had not fallen behind the batch after all (the batch was cut there) */
    uint64_t exchange_words;   /* multi-GPU: u32 words sum-all-reduced for the count deltas of all sequences so far */
    uint32_t exchanges;        /* ... in this many all-reduces (one per sequence) */
    uint32_t log_spilled;      /* "pair_cells": matches that qualified for the delta log but found it full and were counted
                                  with atomics instead (this training) */
    uint64_t fused_live_tokens; /* "time_kernels": live tokens before + live tokens after, summed over the timed fused
                                   passes (x 2 bytes = SURVEY 8(d)'s 2 B x L read + 2 B x L' written of those passes).
                                   In the barrier layout ("chunk_barrier") both terms include one barrier slot per chunk,
                                   which the pass reads and writes like a token; n_live above does not.  Accumulates like
                                   merge_launches */
    float    ms_pair_count_kernel; /* mbpe_pair_count_u8 without a table: mean KERNEL duration of the call's launches
                                   (start/stop events of each dispatch: no gap between launches, no marker overhead) */
    uint32_t log_passes;       /* "pair_cells": stream passes whose count deltas went through the delta log (this training) */
    uint32_t log_refills;      /* "pair_cells": log chunks taken by waves that had filled an earlier one (this training) */
    uint32_t pad3_;
} mbpe_stats;

MBPE_API const char *mbpe_last_error(void);
MBPE_API const char *mbpe_version(void);

/* ---- context ------------------------------------------------------- */

/* Creates a context on HIP device `device_id`.  Fails with
 * MBPE_ERR_NO_DEVICE when there is no such device. */
MBPE_API int  mbpe_create(int device_id, mbpe_ctx **out);
MBPE_API void mbpe_destroy(mbpe_ctx *ctx);

/* ---- corpus -------------------------------------------------------- */

/* Hands the training text to the device.  Replaces text_to_vector +
 * create_lists (Tokenizer.h:85-100, :114-124): the corpus stays a byte
 * array in HBM instead of one heap node per token.
 *   text         n_bytes bytes; host memory, or device memory when
 *                text_on_device != 0 (then it is used in place and must
 *                stay valid until mbpe_train_begin returns)
 *   chunk_off    n_chunks+1 ascending byte offsets, chunk c =
 *                [chunk_off[c], chunk_off[c+1]); chunk_off[0] == 0 and
 *                chunk_off[n_chunks] == n_bytes.  NULL = one chunk = the
 *                whole text (Tokenizer.h:541-544).  Always host memory.
 * Pairs are only counted and merged inside a chunk (Tokenizer.h:135-144,
 * :311-319).  A chunk that starts with NUL and whose remainder parses with
 * std::stoi collapses to one token in the reference (Tokenizer.h:86-93) and
 * therefore never contributes a pair: such chunks are dropped here. */
MBPE_API int mbpe_load_corpus(mbpe_ctx *ctx, const uint8_t *text, uint64_t n_bytes,
                              const uint64_t *chunk_off, uint64_t n_chunks,
                              int text_on_device);

/* The same for a chunked corpus whose chunk ends are already a mask on the device, as mbpe_splitter_split leaves
 * it: endmask_dev = 2 * ceil(n_bytes / 16) + 16 bytes of device memory, 4-byte aligned, bit i & 7 of byte i >> 3 set
 * where text byte i is the last of its chunk, nothing set at or beyond n_bytes.  The mask is copied (device to
 * device) and taken as it is: the chunk count is its population count, taken on the device; no chunk is visited on
 * the host and a device text is not copied back.  The NUL rule of mbpe_load_corpus is the caller's: a chunk the
 * reference collapses to one token must come with every one of its bits set.  (The gpt2 / gpt4 patterns never
 * produce such a chunk: one that starts with NUL holds no ASCII digit, so std::stoi cannot parse its remainder.) */
MBPE_API int mbpe_load_corpus_endmask(mbpe_ctx *ctx, const uint8_t *text, uint64_t n_bytes, int text_on_device,
                                      const uint8_t *endmask_dev);

/* A corpus of chunks with weights: chunk c stands for weights[c] occurrences of its bytes, and every pair count is the
 * weight-sum over the chunks -- the counts of the corpus in which each chunk is written out weights[c] times.  This is
 * how a corpus is trained on its distinct chunks (mbpe_dedup_*, or a word-count table of the caller's).  The result
 * equals the training on the expanded corpus for both tie-breaks, provided that, for `first`, the chunks stand in the
 * order of their first occurrence there.
 *   mbpe_load_corpus_weighted          as mbpe_load_corpus with chunk_off required (NUL rule included); weights: n_chunks
 *                                      u32 of host memory
 *   mbpe_load_corpus_endmask_weighted  as mbpe_load_corpus_endmask (the NUL rule is the caller's); weights: n_weights
 *                                      u32, host memory or, with weights_on_device, device memory (4-byte aligned, copied):
 *                                      what mbpe_dedup_result returns goes in without a host round trip.  n_weights
 *                                      must equal the mask's population count (MBPE_ERR_ARG)
 * A weight of 0, or of 2^31 or more, is MBPE_ERR_ARG (host weights are checked on the host, device weights by a kernel).
 * After such a load
 *   - mbpe_train_begin and mbpe_train_begin_from run on 32-bit tokens (csrc/wide.h) from merge n_prior on, 0 included,
 *     whatever the vocabulary (up to MBPE_MAX_VOCAB_WIDE) and with either tie-break; the options "wide_from",
 *     "first_wide", "resume_wide" and "chunk_barrier" have no effect.  One merge per pass: on a stream of unique chunks
 *     a pass is short, but a large stream trains slowly this way.  Several ranks: MBPE_ERR_STATE.
 *   - a pair whose weighted count reaches 2^31 (or wraps 2^32) is MBPE_ERR_OVERFLOW from the begin; 2^31 - 1 trains
 *   - mbpe_pair_count_u8 returns MBPE_ERR_STATE
 *   - mbpe_train_steps, _train_sequences, _train_result, _get_stream, _get_pairs, _decode_stream and _get_stats behave as
 *     after the handover to 32-bit tokens: stream and decode are those of the chunks that were loaded (the unique
 *     text), counts in _train_result and _get_pairs are the weighted ones.  The zero-count tail (lexical) and the early
 *     end (`first`) are those of the 32-bit loop.
 * Device memory beside that loop's: 4 B per weight, and two u32 arrays of one entry per token. */
MBPE_API int mbpe_load_corpus_weighted(mbpe_ctx *ctx, const uint8_t *text, uint64_t n_bytes, const uint64_t *chunk_off,
                                       uint64_t n_chunks, int text_on_device, const uint32_t *weights);
MBPE_API int mbpe_load_corpus_endmask_weighted(mbpe_ctx *ctx, const uint8_t *text, uint64_t n_bytes, int text_on_device,
                                               const uint8_t *endmask_dev, const uint32_t *weights, uint64_t n_weights,
                                               int weights_on_device);

/* The same for chunks given as ranges [starts[c], ends[c]) (ascending, not overlapping) that need
 * not tile the text: bytes outside every chunk are not part of the corpus, as in the reference's
 * match loop (Tokenizer.h:506-540).  When there are such bytes the library trains on a packed copy
 * of the chunks (host memory, or a device text that is copied back once); mbpe_stats.n_bytes is the
 * packed size. */
MBPE_API int mbpe_load_corpus_ranges(mbpe_ctx *ctx, const uint8_t *text, uint64_t n_bytes,
                                     const uint64_t *starts, const uint64_t *ends, uint64_t n_chunks,
                                     int text_on_device);

/* The pair-count scan on the loaded byte corpus: calculate_freqs
 * (Tokenizer.h:127-146) with PairCountLexicalOrder::create_or_modify_pair
 * (PairCount.h:249-260) as one histogram kernel.  table65536_out (host,
 * optional) receives count[(first << 8) | second].  Test / bench
 * granularity; mbpe_train_begin runs the same kernel.
 * Counts are 32-bit: when a pair occurs 2^32 times or more (its bin
 * wraps), the call returns MBPE_ERR_OVERFLOW and the table it wrote is
 * not valid.  Every count below 2^32 is exact.  (Not checked with
 * "pc_repeat" > 1 and no output table: the timing launches add up.) */
MBPE_API int mbpe_pair_count_u8(mbpe_ctx *ctx, uint32_t *table65536_out);

/* ---- training ------------------------------------------------------ */

/* Prepares the training loop for `vocab_size` (>= 256, Tokenizer.h:492):
 * pair-count scan, 16-bit slot stream, pair table, first argmax.
 * Corresponds to Tokenizer.h:551-556.
 * Pair counts are int32 like the reference's: a byte pair that occurs
 * 2^31 times or more in the corpus returns MBPE_ERR_OVERFLOW, on one GPU
 * here and with several ranks from the exchange that finishes the begin
 * (mbpe_comm_exchange_done; the same decision on every rank), also when
 * the ranks' counts only reach that limit summed, or wrap 2^32 in the
 * u32 all-reduce.  A count of 2^31 - 1 trains. */
MBPE_API int mbpe_train_begin(mbpe_ctx *ctx, uint32_t vocab_size);

/* Runs up to n_steps iterations of the loop body Tokenizer.h:557-589:
 * get_top_pair_count (PairCount.h:262-269), merge_chunks ->
 * merge_incremental (Tokenizer.h:309-320, :202-306).  Stops early when the
 * target vocab size is reached or the pair table is empty (:586-588).
 * steps_done_out (optional) receives the number of merges made by this
 * call. */
MBPE_API int mbpe_train_steps(mbpe_ctx *ctx, uint32_t n_steps, uint32_t *steps_done_out);

/* Runs up to n_sequences *batch sequences*, the unit the library executes: select the next
 * maxima that are provably independent (get_top_pair_count, PairCount.h:262-269, for up to
 * "max_batch" consecutive iterations) -> one pass over the token stream that merges them all
 * (merge_chunks, Tokenizer.h:309-320) -> validate against the one-at-a-time order -> apply the
 * count updates (Tokenizer.h:239-280).  Every sequence commits at least one merge of the loop
 * Tokenizer.h:557-589 unless training is complete; merges_done_out (optional) receives the
 * number this call committed.  With "multi_merge" 0 a sequence is one merge. */
MBPE_API int mbpe_train_sequences(mbpe_ctx *ctx, uint32_t n_sequences, uint32_t *merges_done_out);

/* Copies the merges made so far: merges_out[2k], merges_out[2k+1] is the
 * pair that became token 256+k (Tokenizer.h:578); counts_out[k] (optional)
 * is its count when chosen (the verbose line, Tokenizer.h:566-576).
 * cap_merges = capacity of the arrays in merges. */
MBPE_API int mbpe_train_result(mbpe_ctx *ctx, uint32_t *merges_out, int32_t *counts_out,
                               uint32_t cap_merges, uint32_t *n_merges_out);

/* One call = Tokenizer::train's hot path (Tokenizer.h:551-589) for
 * CONFLICT_RESOLUTION::LEXICAL: load + begin + all steps + result.
 * merges_out must hold 2*(vocab_size-256) u32. */
MBPE_API int mbpe_train_lexical(mbpe_ctx *ctx, const uint8_t *text, uint64_t n_bytes,
                                const uint64_t *chunk_off, uint64_t n_chunks,
                                uint32_t vocab_size,
                                uint32_t *merges_out, int32_t *counts_out,
                                uint32_t *n_merges_out, mbpe_stats *stats_out);

/* The same for either CONFLICT_RESOLUTION of Tokenizer::train (minbpe-cc.cpp:129-131):
 * conflict_resolution 1 = LEXICAL (what mbpe_train_lexical runs), 0 = FIRST -- the reference
 * CLI's default: among the pairs of maximal count the one inserted first into a table rebuilt
 * before every merge wins (PairCountInsertOrder, PairCount.h:65-74, :141-152; recount
 * Tokenizer.h:581-585), i.e. the one whose first occurrence in the corpus comes first.  The
 * device keeps the exact counts incrementally and settles ties with one pass over the stream
 * that finds the earliest position of a tied pair; one merge per pass.  On a sharded stream (several ranks) every rank
 * finds the earliest tied pair of its shard and one more small exchange per merge -- the ranks' hits, the lowest rank
 * that has one wins: shards follow each other in rank order -- makes the choice global.
 * With FIRST the loop ends when no pair is left (Tokenizer.h:586-588): n_merges_out may then be
 * smaller than vocab_size - 256.  Step-level use: mbpe_set_option("conflict_resolution", 0)
 * before mbpe_train_begin. */
MBPE_API int mbpe_train(mbpe_ctx *ctx, const uint8_t *text, uint64_t n_bytes,
                        const uint64_t *chunk_off, uint64_t n_chunks, uint32_t vocab_size,
                        int conflict_resolution,
                        uint32_t *merges_out, int32_t *counts_out,
                        uint32_t *n_merges_out, mbpe_stats *stats_out);

/* ---- continuing from existing merges --------------------------------- */

/* Is `merges` a trained table: both sides of merge k below 256 + k, and no pair twice?  The condition under which the
 * encoder's "rank_order" equals applying the merges one after the other (see mbpe_encoder_set_option), and the one
 * mbpe_train_begin_from asks of its prior merges.  Host only, no device.  MBPE_OK, or MBPE_ERR_ARG with a message that
 * names the first offending index.  An empty table is valid. */
MBPE_API int mbpe_merges_check(const uint32_t *merges, uint32_t n_merges);

/* mbpe_train_begin for a training that starts from the merges prior_merges[0 .. n_prior) instead of from raw bytes
 * (a loaded model, an earlier training, a model of another corpus) and adds merges n_prior, n_prior + 1, ... -- tokens
 * 256 + n_prior, ... -- up to vocab_size.  Same call order as mbpe_train_begin (after a load; "conflict_resolution"
 * before it); n_prior == 0 IS mbpe_train_begin.
 *   1. Every chunk of the loaded corpus becomes the token sequence that applying merge 0, 1, ... in order leaves: a
 *      temporary encoder in rank order reads the context's text and end mask in place (chunks the load dropped or
 *      made inert stay so) and is freed before the training buffers are allocated.
 *   2. The pair table is a fresh count of the adjacent pairs of that stream, inside chunks, overlapping positions
 *      included (calculate_freqs, Tokenizer.h:127-146: a a a gives (a, a) = 2); only pairs that occur are members.
 *   3. The loop of Tokenizer.h:557-589 runs from there, unchanged: mbpe_train_steps, _sequences, _get_stream,
 *      _get_pairs, _stream_device, _table_device, _decode_stream, _compact and _get_stats work as after
 *      mbpe_train_begin.
 * On the same corpus, training to V at once and training to V0 < V, then continuing to V, give the same merges and
 * counts for as long as the chosen counts are >= 1: both tie-breaks depend on the current stream and counts alone.
 * They part in the reference's degenerate tail: its table never erases, so once the maximal count is 0 it goes on
 * merging zero-count pairs that history inserted; a continuation cannot know those pairs and ends when no pair is
 * left, like the reference's loop with a table rebuilt at the point of resumption.
 * mbpe_train_result returns the prior merges followed by the new ones, counts_out[k] = -1 for k < n_prior (no count
 * was observed; 0 is a count the reference reports); steps_done_out / merges_done_out count new merges only,
 * mbpe_stats.n_merges all of them, and ms_begin includes the encoder's device time.  n_prior == vocab_size - 256: the
 * begin succeeds, the training is complete, the result is the prior table.
 * Decided before the device is touched: MBPE_ERR_ARG for a table mbpe_merges_check refuses, for n_prior > vocab_size -
 * 256 and for prior_merges NULL; MBPE_ERR_STATE for a context with several ranks (mbpe_comm_init*; "force_exchange");
 * MBPE_ERR_VOCAB, with the option "resume_wide" 0 (the default), when vocab_size (or 256 + n_prior) lies beyond the
 * 16-bit slot format of this corpus -- the 32-bit continuation does not start from existing merges -- and when
 * "wide_from" is set.  MBPE_ERR_OOM, with the encoder's message, for a corpus above the one-piece limit of
 * mbpe_encoder_encode_endmask; the peak of the begin is the replay, about 18.4 bytes of device memory per corpus byte
 * (DESIGN.md 4h).  MBPE_ERR_OVERFLOW for a pair that occurs 2^31 times or more, as from mbpe_train_begin.
 *
 * With "resume_wide" 1 the training may continue on 32-bit tokens (one rank).  vmax: the slot format's limit for this
 * corpus and "chunk_barrier", as mbpe_train_begin computes it; h = vmax - 256, or min("wide_from", vmax - 256) when
 * "wide_from" >= 0: the merge at which the slot stream hands over; T = vocab_size - 256.
 *   slot case, T <= h            everything above, unchanged
 *   mixed case, n_prior < h < T  the begin above on the slot stream up to merge h, where the handover of
 *                                mbpe_train_begin's trainings takes over; chunk ends are kept as mbpe_train_begin
 *                                would keep them for vocab_size
 *   direct case, n_prior >= h    no slot stream: the replay's tokens are the 32-bit stream, the 64-bit-key pair table
 *                                is counted from them (at most 2^30 pairs: MBPE_ERR_OVERFLOW beyond), and the 32-bit
 *                                loop runs from merge n_prior.  Prior ids may need more than 16 bits.  The calls of
 *                                point 3 behave as after a handover; a table that holds no pair at all ends the loop
 *                                (mbpe_train_steps makes fewer steps), in either tie-break
 * Decided before the device is touched, after the argument checks, in this order: MBPE_ERR_STATE for several ranks;
 * MBPE_ERR_VOCAB for vocab_size > MBPE_MAX_VOCAB_WIDE; MBPE_ERR_VOCAB for the `first` tie-break without "first_wide" 1
 * in the mixed or the direct case.  The zero-count divergence above applies unchanged.  A one-chunk corpus replays one
 * pass per prior merge: tens of thousands of passes for a model near 65,000 merges. */
MBPE_API int mbpe_train_begin_from(mbpe_ctx *ctx, uint32_t vocab_size, const uint32_t *prior_merges, uint32_t n_prior);

/* mbpe_train with prior merges: load + mbpe_train_begin_from + all steps + result.  merges_out must hold
 * 2 * (vocab_size - 256) u32 and receives the prior merges first. */
MBPE_API int mbpe_train_from(mbpe_ctx *ctx, const uint8_t *text, uint64_t n_bytes,
                             const uint64_t *chunk_off, uint64_t n_chunks, uint32_t vocab_size,
                             int conflict_resolution, const uint32_t *prior_merges, uint32_t n_prior,
                             uint32_t *merges_out, int32_t *counts_out,
                             uint32_t *n_merges_out, mbpe_stats *stats_out);

MBPE_API int mbpe_get_stats(mbpe_ctx *ctx, mbpe_stats *out);

/* ---- introspection (parity tests) ----------------------------------- */

/* Live tokens of the stream in order (holes removed).  tokens_out may be
 * NULL to query the length.  chunk_end_out (optional, same length) is 1
 * where a token is the last of its chunk. */
MBPE_API int mbpe_get_stream(mbpe_ctx *ctx, uint32_t *tokens_out, uint8_t *chunk_end_out,
                             uint64_t cap, uint64_t *n_out);

/* Device view of the slot stream, for checks that run on the device (tests, bench.py): n_slots
 * slots of slot_bits bits each in device memory, valid until the next training call.  A slot equal
 * to the all-ones value is a hole; end_bit (0 when there is none) is the slot bit that marks the
 * last token of a chunk, the token id is the slot without it; barrier (MBPE_NO_BARRIER when there
 * is none) is the slot value that stands after the last token of every chunk and is no token. */
MBPE_API int mbpe_stream_device(mbpe_ctx *ctx, const void **slots_out, uint64_t *n_slots_out,
                                uint32_t *slot_bits_out, uint32_t *end_bit_out, uint32_t *barrier_out);

/* Device view of the dense pair table (vocab_size <= 32,768 unless "dense_table" is 0; MBPE_ERR_STATE
 * for the hashed layout): 1 << (2 * vshift) u32 cells, cell of (a, b) at
 *   ((((a >> 5) << (vshift - 5)) | (b >> 5)) << 10) | ((a & 31) << 5) | (b & 31),
 * value 0x80000000 | count once the pair was ever inserted (PairCount.h:249-260 never erases), else 0. */
MBPE_API int mbpe_table_device(mbpe_ctx *ctx, const void **cells_out, uint32_t *vshift_out);

/* All pairs ever inserted with their current counts
 * (PairCount::get_all, PairCount.h:271-278; order unspecified).
 * Arrays may be NULL to query the size. */
MBPE_API int mbpe_get_pairs(mbpe_ctx *ctx, uint32_t *first_out, uint32_t *second_out,
                            int32_t *count_out, uint64_t cap, uint64_t *n_out);

/* Forces a stream compaction now (normally triggered by the hole ratio). */
MBPE_API int mbpe_compact(mbpe_ctx *ctx);

/* Tuning knobs (tests force rare paths with them).
 *   "compact_den"   compact when holes * den >= slots (default 16; 0 = never)
 *   "batch"         sequences (or single merges) per host round trip (default 16)
 *   "multi_merge"   1 = several independent merges per stream pass (default), 0 = one
 *   "max_batch"     most merges one pass may take (default and limit 4096; 1024 when the stream
 *                   is sharded over several GPUs, whose exchange grows with it)
 *   "byte_table"    1 = a batch whose pairs are all pairs of raw bytes is looked up in a byte x byte
 *                   table by the stream kernels (default), 0 = always the hashed batch table
 *   "fused_min"     batches of at least this many pairs read the stream once and write
 *                   the merged stream to the second buffer (default 24; frequent pairs
 *                   qualify earlier); 2 = every multi-pair batch, >= 1000 = never
 *   "dense_table"   -1/1 one cell per possible pair when vocab <= 32,768 (default),
 *                   0 = always the hashed pair table
 *   "threshold_select" 1 = choose batches from a gathered, sorted candidate list
 *                   (default), 0 = always walk the argmax bounds pair by pair
 *   "sel_cap"       capacity of the candidate list of the threshold selection (default and
 *                   limit 8192, at least 64; tests lower it to force the overflow path)
 *   "pc_repeat"     mbpe_pair_count_u8 called without an output table launches the scan this many times
 *                   back to back and reports the mean duration in mbpe_stats.ms_pair_count (timing only)
 *   "hier_argmax"   -1 auto / 0 scan every entry / 1 walk the block bounds
 *                   (single-merge mode)
 *   "force_exchange" 1 = take the multi-rank path (rank edges, exchange) even
 *                   with a single rank (tests the RCCL binding on one GPU)
 *   "chunk_barrier" chunk ends of a chunked corpus as barrier slots: -1 (default) when vocab_size
 *                   exceeds MBPE_MAX_VOCAB_ENDBIT, 1 always, 0 never; read by mbpe_train_begin
 *   "first_batches" `first` tie-break only: 1 = pairs whose count no other candidate shares are merged in batches
 *                   like in lexical mode, a pair with a shared count goes alone after the position tie-break; the
 *                   run hands over to the one-merge-per-pass loop when most sequences are such single pairs.
 *                   Default 0 (one merge per pass): same results, and no faster on text.
 *   "conflict_resolution" 1 = lexical tie-break (default), 0 = first (see mbpe_train); before
 *                   mbpe_train_begin only
 *   "time_kernels"  1 = bracket every merge kernel with HIP events on the
 *                   context's stream; totals appear in mbpe_stats
 *   "lockstep"      how the host enqueues batch sequences: 1 = it waits for every selection and enqueues only the
 *                   kernels that sequence needs (one event wait per sequence, ~12 launches instead of ~27), 0 = it
 *                   enqueues whole groups of sequences with every kernel variant and the device decides which work;
 *                   -1 (default): 1 for streams of up to 32 Mi slots on one rank, 0 otherwise.  Same results.
 *   "pair_cells"    a match whose two neighbours are raw bytes, with no other match touching it, costs the stream pass
 *                   one 4-byte record in a log instead of two atomics on its pair's delta rows; three small kernels
 *                   around the pass sort the records into buckets of 64 pairs and count them in LDS (the name is that
 *                   of the byte x byte cell blocks the log replaced).  1 / 0, -1 (default) = for streams of 64 Mi slots
 *                   and more, where the passes of thousands of byte pairs are bound by their atomics; 1 also logs the
 *                   small batches the default leaves alone.  Read by mbpe_train_begin.  Same results.
 *   "log_cap"       records the log holds (0, the default: a sixteenth of the slots, between 2^20 and 2^28: 1 GiB on the
 *                   benchmark, plus a partition buffer of 2 GiB at most).  A wave that finds the log full counts with
 *                   atomics instead (mbpe_stats.log_spilled); tests reach that with a small value.  Read by
 *                   mbpe_train_begin.
 *   "log_chunk"     records a wave of the pass reserves at a time (0, the default: 4,096, less on a small log; rounded
 *                   to multiples of 256, one tile's most, and at most 65,536); read by mbpe_train_begin
 *   "wide_from"     tests: hand over to the 32-bit continuation after this many merges whatever the vocabulary
 *                   (-1, the default: where the 16-bit slot format ends); read by mbpe_train_begin
 *   "first_wide"    `first` tie-break beyond the 16-bit slot format, one rank: 0 (default) = MBPE_ERR_VOCAB, 1 = the
 *                   first vocab_size limit - 256 merges on the slot stream, the rest on 32-bit tokens with the same
 *                   tie-break (earliest first occurrence among the pairs of maximal count), ending when no pair is
 *                   left; read by mbpe_train_begin.  mbpe_train takes what the context says; Tokenizer::train sets 1
 *   "resume_wide"   continuing from existing merges beyond the 16-bit slot format, one rank: 0 (default) =
 *                   MBPE_ERR_VOCAB, 1 = on 32-bit tokens (the mixed and direct cases of mbpe_train_begin_from); any
 *                   other value is MBPE_ERR_ARG.  Read by mbpe_train_begin_from; mbpe_train_from takes what the
 *                   context says; Tokenizer::train sets 1
 *   "min_frequency", "max_token_length"
 *                   the stopping rules of a training; both 0 (the default) = none, and every call does exactly what it
 *                   does without them.  Read by mbpe_train_begin and mbpe_train_begin_from; mbpe_train, _train_lexical
 *                   and _train_from take what the context says.
 *                     "max_token_length" L: 0, or 2 .. 2^31 - 1 bytes.  A token's length is 1 for a byte and the sum of
 *                       its halves' for a merge; the prior merges of a continued training count, whatever their length.
 *                       A pair (a, b) is eligible iff len[a] + len[b] <= L.  Ineligible pairs stay in the stream and
 *                       the table and are counted as ever; they are never chosen, never win a tie and do not make a
 *                       unique eligible maximum a tie.
 *                     "min_frequency" f: 0 .. 2^31 - 1, compared with the (weighted) pair count.
 *                   Any other value is MBPE_ERR_ARG.  One step: M is the largest count among the eligible pairs; the
 *                   training ends when no pair is eligible, when M < f, or (`first`, as ever) when M is 0; otherwise the
 *                   tie-break chooses among the eligible pairs of count M.  The limits apply to the new merges only.  A
 *                   training that ended reports fewer merges than vocab_size - 256 (mbpe_train_result), and
 *                   mbpe_train_steps makes fewer steps, then 0.  With lexical and f = 0 an eligible pair of count 0 is
 *                   chosen again and again, as without limits.
 *                   With either option non-zero the training runs on 32-bit tokens (csrc/wide.h) from merge n_prior
 *                   on, 0 included, like one on a corpus with chunk weights: weighted or not, either tie-break, any
 *                   vocabulary up to MBPE_MAX_VOCAB_WIDE (beyond: MBPE_ERR_VOCAB); "wide_from", "first_wide",
 *                   "resume_wide" and "chunk_barrier" play no part.  Several ranks, "force_exchange" included:
 *                   MBPE_ERR_STATE.  The text is widened by the rank-ordered replay of mbpe_train_begin_from, so a
 *                   corpus above the encoder's one-piece limit is MBPE_ERR_OOM.  The rules live in that loop's argmax,
 *                   on the device; the 16-bit slot stream's batched selection does not know them.  So a limited training
 *                   makes one pass over the loaded corpus per merge: load the distinct chunks with their counts
 *                   (mbpe_dedup_*, mbpe_load_corpus_*_weighted), or it is correct and slow.  The route is never
 *                   switched beyond this.  Device memory beside the loop's: 4 B per token id for the lengths.
 */
MBPE_API int mbpe_set_option(mbpe_ctx *ctx, const char *name, int64_t value);

/* ---- encode on the device ----------------------------------------------- */

/* internal_encode (Tokenizer.h:370-377) over all chunks of a text on HIP device `device_id`:
 * every chunk is widened with text_to_vector (Tokenizer.h:85-100, including its rule that a chunk
 * starting with NUL whose remainder parses with std::stoi is ONE token with that id -- how encode
 * hands over special tokens, :635-637, :667-670) and run through internal_internal_encode
 * (:325-367): left-to-right passes that replace ANY pair present in merges_lookup, until a pass
 * replaces nothing.  The results are concatenated (:713-717).
 *   text, chunk_off, n_chunks   as for mbpe_load_corpus (host memory; NULL chunk_off = one chunk)
 *   merges                      2 * n_merges u32, merge k makes token 256 + k; a repeated pair keeps
 *                               the last id (merges_lookup[pair] = idx, Tokenizer.h:579)
 *   tokens_out                  may be NULL to query the count; cap = its capacity in tokens
 *   n_out                       required.  Receives the token count whenever the passes ran: with tokens_out NULL, and
 *                               when cap is smaller -- then the call returns MBPE_ERR_ARG and writes no token.  An argument
 *                               refused before the passes (NULL text or merges with a count, chunk_off not ascending from
 *                               0 to n_bytes, a NUL-led chunk's id) leaves 0 there
 *   n_passes_out                optional: stream passes made (1 + the replacing passes of the deepest chunk; 0 for an
 *                               empty text), reported together with n_out
 * No CPU fallback: MBPE_ERR_NO_DEVICE without a HIP device.  Token ids must stay below 2^31 - 2. */
MBPE_API int mbpe_encode_chunks(int device_id, const uint8_t *text, uint64_t n_bytes,
                                const uint64_t *chunk_off, uint64_t n_chunks,
                                const uint32_t *merges, uint32_t n_merges,
                                uint32_t *tokens_out, uint64_t cap, uint64_t *n_out,
                                uint32_t *n_passes_out);

/* The same with the result left on the device: tokens_dev_out is device memory of `device_id` for cap tokens
 * (NULL to query the count) and receives the tokens as the passes leave them, bit 31 = last token of its chunk
 * (mask with 0x7FFFFFFF for the id; mbpe_decode_slots with slot_bits 32 and end_bit 0x80000000 reads them as they
 * are). */
MBPE_API int mbpe_encode_chunks_device(int device_id, const uint8_t *text, uint64_t n_bytes,
                                       const uint64_t *chunk_off, uint64_t n_chunks,
                                       const uint32_t *merges, uint32_t n_merges,
                                       uint32_t *tokens_dev_out, uint64_t cap, uint64_t *n_out,
                                       uint32_t *n_passes_out);

/* An encoder: the same encode as an object that is created once per merges table and called many times.  It keeps,
 * on HIP device `device_id`, the pair -> id lookup table, its own non-blocking stream and the work buffers (about 13
 * bytes per text byte of the largest piece encoded so far); a call that needs larger buffers grows them, any other
 * call allocates nothing.  The two calls above are a temporary encoder plus one mbpe_encoder_encode.
 * Arguments are checked, and the table is built, before the device is touched.  No CPU fallback: MBPE_ERR_NO_DEVICE
 * without a HIP device.  Thread-compatible like a context: one call at a time. */
typedef struct mbpe_encoder mbpe_encoder;
MBPE_API int  mbpe_encoder_create(int device_id, const uint32_t *merges, uint32_t n_merges, mbpe_encoder **out);
MBPE_API void mbpe_encoder_destroy(mbpe_encoder *e);

/* Encodes all chunks of a text.
 *   text               n_bytes bytes; host memory, or -- text_on_device != 0 -- device memory of the encoder's device,
 *                      which is read in place and never written.  (The chunks of a device text that start with NUL
 *                      are found by a kernel and copied back for the std::stoi rule; results and error codes are those
 *                      of a host text.)
 *   chunk_off, n_chunks  as for mbpe_encode_chunks; always host memory
 *   tokens_out         cap tokens of token_bits bits each: host memory, or device memory when out_on_device != 0.
 *                      token_bits 32, host: uint32_t ids.  token_bits 32, device: bit 31 = last token of its chunk,
 *                      as mbpe_encode_chunks_device leaves them.  token_bits 16: uint16_t ids without flags, host or
 *                      device; MBPE_ERR_VOCAB, before any pass runs, when 256 + n_merges > 65,536 or a NUL-led chunk
 *                      names an id >= 65,536.  Any other token_bits is MBPE_ERR_ARG.
 *                      NULL: query.  n_out receives the count whenever the passes ran; a cap that is too small
 *                      returns MBPE_ERR_ARG, writes no token (and no chunk offset beyond [0]) and still reports the
 *                      count.  cap = n_bytes always suffices: encoding never makes more tokens than bytes.
 *   chunk_tok_off_out  optional, host, n_chunks + 1 entries: the tokens of chunk c are
 *                      [chunk_tok_off_out[c], chunk_tok_off_out[c + 1]) of the output; [0] == 0, [n_chunks] == *n_out,
 *                      an empty chunk repeats its predecessor's offset.  Also filled by a query.  NULL: the chunk ends
 *                      are neither computed nor stored.
 *   n_passes_out       optional: stream passes made (of the piece that needed most)
 * Pieces: a text longer than the option "piece_bytes" is cut at chunk boundaries into pieces of at most that many
 * bytes (greedily: every piece takes as many whole chunks as fit), which go through the same buffers one after the
 * other; tokens and offsets are appended, the result is that of the unsplit call.  A single chunk longer than a piece
 * returns MBPE_ERR_OOM with a message that names it; the encoder stays usable.  With "piece_bytes" 0 (the default) a
 * text that fits the buffers the encoder already holds is one piece; otherwise the limit is
 * (free + held - (free + held) / 16) / 14 bytes, where free is the device memory hipMemGetInfo reports at the call
 * and held the size of the encoder's work buffers: a piece costs 13.2 bytes of device memory per text byte
 * (with token byte offsets for the host: up to 21.2, and the divisor is 22 -- see mbpe_encoder_encode_byteoff).
 * While dropout is on (mbpe_encoder_set_dropout) a piece costs 8 bytes per text byte more, the two arrays of byte
 * starts: the divisor is 22 instead of 14, with byte offsets for the host 30 instead of 22, and a piece holds at most
 * 2^32 bytes whatever "piece_bytes" says, because a byte start is 32 bits.
 * When the pieces are several and cap < n_bytes, the passes run twice (count first, so that a cap too small writes
 * nothing). */
MBPE_API int  mbpe_encoder_encode(mbpe_encoder *e, const uint8_t *text, uint64_t n_bytes, int text_on_device,
                                  const uint64_t *chunk_off, uint64_t n_chunks,
                                  void *tokens_out, uint64_t cap, uint32_t token_bits, int out_on_device,
                                  uint64_t *chunk_tok_off_out, uint64_t *n_out, uint32_t *n_passes_out);

/*   "piece_bytes"   the most text bytes encoded in one go; 0 (default) = chosen at the call, see above.
 *   "rank_order"    the order in which the merges are applied to a chunk.  0 (default): the reference's greedy passes
 *                   (Tokenizer.h:325-367: a left-to-right pass replaces ANY pair it finds in the lookup, first match
 *                   wins).  1: rank order.  Per chunk, after text_to_vector: of the adjacent pairs that are in the
 *                   lookup (a repeated pair keeps the last id) take the smallest id m; stop when there is none;
 *                   replace every occurrence of that pair with m, left to right and non-overlapping (a a a with (a,a)
 *                   gives m a); repeat.  For a table in which both sides of merge k are below 256 + k and no pair
 *                   occurs twice -- every trained model -- that equals applying merges 0 .. n-1 in order: the
 *                   segmentation the trainer left in its stream (mbpe_get_stream) and what other BPE implementations
 *                   give for the same merges.  For any other table the loop above is the definition.
 *                   The option holds for mbpe_encoder_encode, _encode_batch, _encode_batch_aux, _encode_endmask and
 *                   _encode_batch_endmask, with everything else (pieces, 16-bit output, device text, queries, cap
 *                   rules, NUL-led chunks, singles) as it is; mbpe_encode_chunks* stay greedy.  Any value but 0 and 1
 *                   is MBPE_ERR_ARG.
 *                   Passes: a device pass applies, in every chunk at once, that chunk's smallest candidate id, so
 *                   n_passes_out is 1 + the most rounds any chunk needs.  That is not capped: a chunk of L tokens
 *                   needs at most L passes, a text that is ONE chunk one pass per distinct merge that applies (the
 *                   whole table, for the text a basic model was trained on), where the greedy order needs a
 *                   handful.  With the gpt2 / gpt4 split at vocab 512: 9-14 passes against 4.  Every pass is a few
 *                   short kernels and one 8-byte read-back, as in the default order; mbpe_encoder_pass_tokens reports
 *                   them.  The option adds 20 bytes per 1,024 text bytes to the work buffers, allocated when the
 *                   first call in rank order needs them.
 * An unknown name or a negative value is MBPE_ERR_ARG. */
MBPE_API int  mbpe_encoder_set_option(mbpe_encoder *e, const char *name, int64_t value);

/* BPE-dropout (Provilkov et al., 2020; the `dropout` of other tokenizers' BPE models) in rank order: a merge that
 * applies is skipped with probability p, so the same text gets another segmentation with every seed.
 * Definition.  Rank order only.  Per chunk, after text_to_vector, repeat: of the adjacent pairs (t[i], t[i + 1]) that
 * are in the lookup AND whose instance is not dropped take the smallest merged id m; stop when there is none; replace
 * the surviving instances of m, left to right and non-overlapping.  An INSTANCE is (pos, id): pos = the offset of the
 * first byte of t[i] in the buffer the encoder read -- 64 bits, over the whole call, not over a piece or a chunk --
 * and id = the merged token.  It is dropped iff drop_hash(seed, pos, id) < threshold, threshold in [0, 2^32]:
 *     x  = seed + pos * 0x9E3779B97F4A7C15 + (uint64_t)id * 0xD1B54A32D192ED03           (mod 2^64)
 *     x ^= x >> 30;  x *= 0xBF58476D1CE4E5B9;  x ^= x >> 27;  x *= 0x94D049BB133111EB;  x ^= x >> 31
 *     drop_hash = x >> 32
 * A pure function of (seed, pos, id): an instance that is dropped stays dropped in every later round, and the result
 * does not depend on pieces, spans or the other chunks; a CPU loop reproduces it bit for bit.  threshold 2^32 (p = 1)
 * leaves the bytes, threshold 0 is plain rank order.  In a run a a a with (a,a) whose instance at 0 is dropped, the
 * instance at 1 is replaced: the left-to-right rule runs over the surviving candidates.  Chunks that are one token by
 * rule (NUL-led with a number, mbpe_single) have no candidates and are never touched.
 *   mbpe_dropout_threshold    floor(p * 2^32), exact for p = 0 and p = 1; NaN or a p outside [0, 1]: MBPE_ERR_ARG
 *   mbpe_encoder_set_dropout  holds from the next call on for mbpe_encoder_encode, _encode_batch, _encode_batch_aux,
 *                             _encode_endmask, _encode_batch_endmask and the _byteoff calls (whose offsets come from
 *                             the final stream, as without dropout).  A threshold above 2^32 is MBPE_ERR_ARG.
 * An encode call with threshold > 0 while "rank_order" is 0 returns MBPE_ERR_ARG with a message, before the device is
 * touched; the encoder stays usable and the order is never switched silently.  mbpe_encode_chunks* and the replay
 * inside mbpe_train_begin_from never drop.
 * How: every token carries the byte start of its first byte through the passes (32 bits, relative to the piece, beside
 * the two token arrays; a merged token keeps its left token's), the candidate kernel reads it where the lookup hit and
 * clears a dropped candidate before the rank kernels see it; every kernel after that is the plain one.  With threshold
 * 0 the launches, the buffers and mbpe_encoder_alloc_count are exactly those of an encoder that never heard of
 * dropout; the 8 bytes per text byte are reserved by the first call that needs them (see "Pieces" above). */
MBPE_API int  mbpe_dropout_threshold(double p, uint64_t *threshold_out);
MBPE_API int  mbpe_encoder_set_dropout(mbpe_encoder *e, uint64_t threshold, uint64_t seed);

/* Device time of the encoder's latest call in milliseconds: HIP events on its stream around widen, the passes (with
 * the 8-byte read-back that ends each) and the finishing kernels (those of the token byte offsets included), summed
 * over the pieces; the copies of text, mask and output between host and device are outside.  Where the passes ran
 * twice (several pieces and cap < n_bytes) both runs are in it. */
MBPE_API int  mbpe_encoder_kernel_ms(const mbpe_encoder *e, float *ms_out);

/* The passes of the latest call: tokens_out[k] = tokens that entered pass k, summed over the pieces ([0] = n_bytes;
 * of passes that ran twice, one run).
 * tokens_out NULL: n_out receives how many there are.  For the byte accounting of tools/encode_time.py. */
MBPE_API int  mbpe_encoder_pass_tokens(const mbpe_encoder *e, uint64_t *tokens_out, uint32_t cap, uint32_t *n_out);

/* Device allocations (hipMalloc calls) the encoder has made since it was created, the lookup table's included.  A
 * call on a text no longer than an earlier one, with the same arguments, leaves the number as it is.  (Three small
 * buffers follow other sizes and may still grow then: the list of NUL-led chunks with their number, and a list of
 * chunk ends of its own when chunks are shorter than two bytes on average -- otherwise the ends borrow the idle
 * token array.  A call with token byte offsets has three more: len[], once; the singles' token indices; and, for
 * host output, the staging buffer that follows the TOKEN count of the largest piece.) */
MBPE_API int  mbpe_encoder_alloc_count(const mbpe_encoder *e, uint64_t *n_out);

/* ---- encode through the unique chunks (csrc/expand.hip, expand.h) --------------------------------------------------
 * mbpe_encoder_set_option(e, "dedup", 0 | 1), default 0; any other value is MBPE_ERR_ARG.  With 0 the encoder launches
 * and allocates exactly what it does without the option: no deduper exists and mbpe_encoder_alloc_count is unchanged.
 * With 1, mbpe_encoder_encode, _encode_batch, _encode_batch_aux, _encode_endmask and _encode_batch_endmask give the same
 * tokens, offsets, matrices and error codes on another route.  Without dropout a chunk's tokens depend on its bytes
 * alone, in both orders, so:
 *   1. the encoder's own deduper (mbpe_dedup_*, created by the first such call, option "map" on) finds the unique chunks
 *      of the call's text and mask (the endmask calls) or text and chunk_off (host or device text; a device text that
 *      is not 16-byte aligned is copied once);
 *   2. the existing passes, greedy or rank order, run over the unique text and its end mask as ONE piece, without any
 *      single and without the NUL rule: a NUL-led chunk's bytes there are ordinary bytes that nothing points at;
 *   3. the finishing kernel writes them into a kept table in the caller's format (32 bits with bit 31 on a chunk's last
 *      token, plain 32 bits, 16 bits) with every run's end; the chunks that are one token by rule (NUL-led with a number,
 *      mbpe_single) become runs of their own behind them;
 *   4. the expansion copies every chunk's run to its place: a 64-bit token count per span of 1,024 chunks, one scan,
 *      the total read back BEFORE anything is written (a cap that is too small writes nothing and still reports the
 *      count), then one wave per span that walks the span's output in pieces of 16 aligned bytes.  The chunks' token
 *      offsets (chunk_tok_off_out, the batch calls' documents) and the endmask calls' document offsets come from the
 *      same sums; the latter stay on the device for the pack kernel.
 * Pieces: the call's text is one piece for the deduper, and the unique text is one piece under the limit of
 * mbpe_encoder_encode (option "piece_bytes"); a unique text above it returns MBPE_ERR_OOM with a message that names both
 * numbers, and the encoder stays usable.  Device memory: the deduper's (see mbpe_dedup_*: 1 1/8 B per text byte of a host
 * text, 44 .. 68 B per chunk with the map, 8 B more per chunk where chunk_off has empty chunks), the pieces' 14 B per
 * UNIQUE byte, the table (4 or 2 B per unique token, 8 B per unique chunk and per one-token chunk), 8 B per 1,024 chunks,
 * 8 B per chunk where the chunks' token offsets are asked for (the batch calls), the output's size once more when it
 * goes to the host, and for the endmask calls with singles or documents 12 B per 2,048 text bytes.
 * Refused, before the device is touched, with MBPE_ERR_ARG: any of these calls while mbpe_encoder_set_dropout has a
 * threshold above 0 (a dropped instance depends on its position, so equal chunks do not share their tokens), and the
 * _byteoff calls with a tok_byte_off_out that is not NULL (with NULL they are their counterparts, as ever); a device
 * tokens_out that is not aligned to its elements.  The route is never switched silently.
 *   "dedup_max_chunk_bytes"  forwards to the deduper's "max_chunk_bytes" (default 256; 0 .. 2^31 - 1): a longer chunk
 *                            passes through as a unique chunk every time it occurs, which is as exact
 * mbpe_encode_chunks* and the replay inside mbpe_train_begin_from never take this route.
 * mbpe_encoder_pass_tokens then reports the passes over the unique text ([0] = its byte count), mbpe_encoder_kernel_ms
 * the deduper's kernels, the passes, the finishing kernel and the expansion.  A repeat call of no larger size allocates
 * nothing.
 *   mbpe_encoder_dedup_stats  the latest call: the chunks the deduper kept, the unique chunks, their bytes, the tokens they
 *                             became (the table without the one-token chunks) and the device time of the expansion
 *                             (chunk look-ups, count, scan, copy); any pointer may be NULL.  MBPE_ERR_STATE when the
 *                             latest call did not take this route.
 * Use it for large texts in natural language (few distinct chunks), above all in rank order, whose many passes then
 * run over a few hundred kilobytes; do not use it where most chunks are distinct or the text is one chunk: the dedup
 * and the copy come on top of the same passes (README, "Encoding through the unique chunks"). */
MBPE_API int  mbpe_encoder_dedup_stats(const mbpe_encoder *e, uint64_t *n_chunks_out, uint64_t *n_unique_out,
                                       uint64_t *n_unique_bytes_out, uint64_t *n_unique_tokens_out, float *expand_ms_out);

/* ---- fixed-length id matrices --------------------------------------------- */

/* A model input is a rectangle: [rows, seq_len] ids plus one length per row.  These calls build it on the device
 * from a flat token stream with per-document offsets -- what mbpe_encoder_encode leaves there -- and take it back
 * (csrc/pack.hip).  Let nb / ne be 1 where bos_id / eos_id is set, else 0.
 *   MBPE_PACK_PADDED  one row per document: [bos] body [eos], where body is the document's first keep = seq_len - nb
 *                     - ne tokens (its last keep with trunc_left); len = nb + |body| + ne; the row is filled with
 *                     pad_id up to seq_len on the right, or -- pad_left -- on the left.  An empty document gives a row
 *                     of len nb + ne.  n_rows = n_docs.
 *   MBPE_PACK_PACKED  the stream S = the concatenation over the documents of [bos] doc [eos], cut row-major into
 *                     ceil(|S| / seq_len) rows; the tail of the last row is pad_id; len[r] = elements of S in row r.
 *                     pad_left and trunc_left must be 0.
 * Like the encoder and the decoder these calls work on a stream of their own and return when the matrix is complete:
 * device buffers handed to them must not be in use by work still in flight on another stream. */
#define MBPE_PACK_PADDED 0u
#define MBPE_PACK_PACKED 1u
#define MBPE_NO_TOKEN 0xFFFFFFFFu
typedef struct {
    uint32_t layout;      /* MBPE_PACK_PADDED or MBPE_PACK_PACKED */
    uint32_t seq_len;     /* ids per row, at least 1 */
    uint32_t out_bits;    /* 16, 32 or 64: uint16_t / uint32_t / uint64_t ids (the last is what an int64 tensor takes) */
    uint32_t pad_id;
    uint32_t bos_id;      /* MBPE_NO_TOKEN: none */
    uint32_t eos_id;      /* MBPE_NO_TOKEN: none */
    uint32_t pad_left;    /* PADDED: 0 = the padding follows the ids, otherwise it comes first */
    uint32_t trunc_left;  /* PADDED: 0 = a document too long keeps its first tokens, otherwise its last */
} mbpe_pack_spec;

/* One call, with its own device scratch for the offsets (and for whatever lives on the host).
 *   tokens, n_tokens, token_bits, tokens_on_device   the ids: host or device memory.  token_bits 32: uint32_t whose
 *                     bit 31 is cleared on read, so that host ids and the flagged tokens mbpe_encoder_encode leaves on
 *                     the device are both accepted.  token_bits 16: plain uint16_t ids, 65,535 included
 *   doc_tok_off, n_docs   host; the convention of mbpe_decode_batch: n_docs + 1 ascending offsets, [0] == 0,
 *                     [n_docs] == n_tokens
 *   ids_out           cap_rows rows of spec->seq_len ids of spec->out_bits bits, row-major without gaps: host memory,
 *                     or device memory (aligned to one id) when out_on_device != 0.  NULL: query
 *   len_out           optional: one uint32_t per row, on the same side as ids_out
 *   n_rows_out        required; written whenever the arguments are valid.  cap_rows smaller than it returns
 *                     MBPE_ERR_ARG and writes nothing else
 * MBPE_ERR_ARG: a NULL argument, a bad offset array, seq_len == 0, seq_len < nb + ne (PADDED), an unknown layout or
 * bit width, pad_left or trunc_left with PACKED.  MBPE_ERR_VOCAB: out_bits 16 with token_bits 32, or with a pad_id,
 * bos_id or eos_id >= 65,536.  All of it is checked, and a query answered, before the device is touched.  No CPU
 * fallback: MBPE_ERR_NO_DEVICE without a HIP device. */
MBPE_API int  mbpe_pack_tokens(int device_id, const void *tokens, uint64_t n_tokens, uint32_t token_bits,
                               int tokens_on_device, const uint64_t *doc_tok_off, uint64_t n_docs,
                               const mbpe_pack_spec *spec, void *ids_out, uint64_t cap_rows, int out_on_device,
                               uint32_t *len_out, uint64_t *n_rows_out);

/* The inverse of a right-padded PADDED matrix: row r contributes its first len[r] ids.
 *   ids, n_rows, seq_len, id_bits, ids_on_device   the matrix (id_bits 16, 32 or 64; ids stay below 2^31) and, on the
 *                     same side, len: one uint32_t per row.  The lengths of a device matrix are copied back first
 *   tokens_out        cap tokens of token_bits bits (16 only with id_bits 16, else MBPE_ERR_VOCAB; 32), host or device
 *                     (out_on_device): the rows' ids one after the other.  NULL: query
 *   doc_tok_off_out   optional, host, n_rows + 1 entries: row r is tokens [doc_tok_off_out[r], doc_tok_off_out[r + 1]).
 *                     Together with tokens_out on the device this is what mbpe_decode_batch takes, as it is
 *   n_out             required: the token count, also on a query and when cap is too small (MBPE_ERR_ARG, nothing
 *                     written to tokens_out)
 * A len[r] above seq_len is MBPE_ERR_ARG. */
MBPE_API int  mbpe_unpack_tokens(int device_id, const void *ids, uint64_t n_rows, uint32_t seq_len, uint32_t id_bits,
                                 int ids_on_device, const uint32_t *len, void *tokens_out, uint64_t cap,
                                 uint32_t token_bits, int out_on_device, uint64_t *doc_tok_off_out, uint64_t *n_out);

/* Device time in milliseconds of the kernel of the calling thread's latest mbpe_pack_tokens or mbpe_unpack_tokens
 * (HIP events around it; allocations and copies are outside). */
MBPE_API int  mbpe_pack_kernel_ms(float *ms_out);

/* Encode and pack in one call: mbpe_encoder_encode into a flat device buffer that the encoder keeps (allocated by
 * the first such call, grown like the work buffers: a repeat call of no larger size leaves
 * mbpe_encoder_alloc_count as it is), then the pack kernel on the encoder's own stream.  No token crosses to the
 * host; only the chunk ends do.
 *   text .. n_chunks  as for mbpe_encoder_encode (pieces included)
 *   doc_chunk_off, n_docs   host, n_docs + 1 ascending chunk indices from 0 to n_chunks: document i is the chunks
 *                     [doc_chunk_off[i], doc_chunk_off[i + 1])
 *   spec .. n_rows_out   as for mbpe_pack_tokens, for tokens of 16 bits when spec->out_bits is 16 (MBPE_ERR_VOCAB when
 *                     256 + n_merges > 65,536) and of 32 bits otherwise.  A query (ids_out NULL) runs the passes
 *   n_tokens_out      optional: tokens encoded, before bos, eos, truncation and padding
 * mbpe_encoder_kernel_ms then covers both steps, mbpe_encoder_pack_ms the pack kernel alone. */
MBPE_API int  mbpe_encoder_encode_batch(mbpe_encoder *e, const uint8_t *text, uint64_t n_bytes, int text_on_device,
                                        const uint64_t *chunk_off, uint64_t n_chunks,
                                        const uint64_t *doc_chunk_off, uint64_t n_docs, const mbpe_pack_spec *spec,
                                        void *ids_out, uint64_t cap_rows, int out_on_device, uint32_t *len_out,
                                        uint64_t *n_rows_out, uint64_t *n_tokens_out);
MBPE_API int  mbpe_encoder_pack_ms(const mbpe_encoder *e, float *ms_out);

/* ---- training batches: labels, positions, segments, cu_seqlens ------------ */

/* What a training step needs beside the ids, written by the same kernel from the same walk (k_pack_aux,
 * csrc/pack.hip).  A document as it appears in the matrix is the element list E_d = [bos] body [eos] with
 * T_d = |E_d|: for MBPE_PACK_PACKED body is the whole document d, which may span rows; for MBPE_PACK_PADDED it is the
 * kept (truncated) part, T_d = len[d], in columns [lead, lead + T_d) of row d.  Every cell of the matrix is a pad cell
 * or holds element k of some E_d:
 *   labels  [n_rows, seq_len] ids of spec->out_bits bits: E_d[k + 1] if k + 1 < T_d, else ignore_label; ignore_label
 *           in a pad cell.  A label never crosses a document: with eos set the token before it has label eos and eos
 *           itself ignore_label.  In PACKED a label does cross a row end inside a document
 *   pos     [n_rows, seq_len] uint32_t: k (it goes on counting in a document that continues in the next row); 0 in a
 *           pad cell
 *   seg     [n_rows, seq_len] uint32_t: d + 1, d the document's number among all n_docs; 0 in a pad cell.  An empty
 *           document without bos / eos occupies no cell: its number is skipped
 * ignore_label is written truncated to out_bits: -100 comes out as -100 in an int64 / int32 tensor.  With out_bits 16
 * it must lie in 0 .. 65,535 (MBPE_ERR_VOCAB), with out_bits 32 in -2^31 .. 2^32 - 1 (MBPE_ERR_ARG).  seg needs
 * n_docs < 2^32 - 1 and pos, in PACKED, every T_d < 2^32 (MBPE_ERR_ARG). */
typedef struct {
    void     *labels;        /* [n_rows, seq_len] ids of spec->out_bits bits, or NULL */
    uint32_t *pos;           /* [n_rows, seq_len], or NULL */
    uint32_t *seg;           /* [n_rows, seq_len], or NULL */
    int64_t   ignore_label;
} mbpe_pack_aux;             /* on the same side as ids_out */

/* mbpe_pack_tokens with the outputs of `aux` (required: NULL is MBPE_ERR_ARG; all three of its pointers NULL is
 * valid and gives ids and lengths alone, equal to those of mbpe_pack_tokens).  Every other argument, the query
 * (ids_out NULL) and the cap rule are those of mbpe_pack_tokens, except that with out_on_device each of ids_out,
 * labels, pos and seg that is given must be 16-byte aligned (MBPE_ERR_ARG).  Host outputs go through device buffers
 * of the call's own and come back with the ids.  All arguments are checked before the device is touched; an error
 * return writes nothing.  mbpe_pack_kernel_ms covers this kernel too. */
MBPE_API int  mbpe_pack_tokens_aux(int device_id, const void *tokens, uint64_t n_tokens, uint32_t token_bits,
                                   int tokens_on_device, const uint64_t *doc_tok_off, uint64_t n_docs,
                                   const mbpe_pack_spec *spec, void *ids_out, uint64_t cap_rows, int out_on_device,
                                   uint32_t *len_out, uint64_t *n_rows_out, const mbpe_pack_aux *aux);

/* cu_seqlens and max_seqlen of a MBPE_PACK_PACKED matrix for variable-length attention, on the host alone (no device,
 * never MBPE_ERR_NO_DEVICE).  With n_stream = doc_tok_off[n_docs] + n_docs * (nb + ne) the list is, ascending and
 * without duplicates: the row starts r * seq_len < n_stream, the document starts doc_tok_off[d] + d * (nb + ne), and
 * n_stream -- the boundaries of the maximal runs of cells with equal (row, seg) in the flattened matrix.  Empty
 * documents vanish, the pad tail behind n_stream is outside, n_stream == 0 gives [0] and n_seqs 0.
 *   doc_tok_off, n_docs   as for mbpe_pack_tokens (what mbpe_encoder_encode_batch_aux hands back)
 *   cu_out            cap_seqs + 1 entries, host.  NULL: query
 *   n_seqs_out, max_seqlen_out   required: the sequences (the list has n_seqs + 1 entries) and the longest of them,
 *                     at most seq_len; also on a query and when cap_seqs is too small (MBPE_ERR_ARG, nothing written)
 * MBPE_ERR_ARG also for MBPE_PACK_PADDED (there the sequences are the rows, and mbpe_unpack_tokens gives their
 * offsets) and for n_stream >= 2^31. */
MBPE_API int  mbpe_pack_cu_seqlens(const uint64_t *doc_tok_off, uint64_t n_docs, const mbpe_pack_spec *spec,
                                   int32_t *cu_out, uint64_t cap_seqs, uint64_t *n_seqs_out, uint32_t *max_seqlen_out);

/* mbpe_encoder_encode_batch with the outputs of `aux` (rules as for mbpe_pack_tokens_aux; host outputs go through
 * buffers the encoder keeps, so a repeat call of no larger size leaves mbpe_encoder_alloc_count as it is).
 *   doc_tok_off_out   optional, host, n_docs + 1 entries: the token offsets of the documents, which the host has
 *                     after the encode -- what mbpe_pack_cu_seqlens takes.  Written on a query too
 * The limits on T_d (pos, PACKED) are checked after the encode passes, before the pack kernel.
 * mbpe_encoder_pack_ms covers this kernel too. */
MBPE_API int  mbpe_encoder_encode_batch_aux(mbpe_encoder *e, const uint8_t *text, uint64_t n_bytes, int text_on_device,
                                            const uint64_t *chunk_off, uint64_t n_chunks,
                                            const uint64_t *doc_chunk_off, uint64_t n_docs, const mbpe_pack_spec *spec,
                                            void *ids_out, uint64_t cap_rows, int out_on_device, uint32_t *len_out,
                                            uint64_t *n_rows_out, uint64_t *n_tokens_out, const mbpe_pack_aux *aux,
                                            uint64_t *doc_tok_off_out);

/* ---- encode from an end mask that is on the device ----------------------- */

/* mbpe_encoder_encode for a text and an end mask that both are device memory of the encoder's device already -- what
 * mbpe_splitter_split_docs leaves behind (mbpe_splitter_endmask).  Both are read in place.
 *   text_dev, n_bytes   the text
 *   endmask_dev         its end mask in the splitter's and the trainer's layout (bit i & 7 of byte i >> 3 = text byte i
 *                       is the last of its chunk; 2 * ceil(n_bytes / 16) + 16 bytes, nothing set at or beyond n_bytes),
 *                       4-byte aligned
 *   singles, n_singles  host, ascending and disjoint: bytes [start, start + len) are ONE token, `id`.  The text holds
 *                       the special tokens' names, not "\0<id>" markers, and no chunk is parsed for a number: the
 *                       caller says which ranges are single tokens.  Checked on the host: order, range, and that every
 *                       id fits the output (MBPE_ERR_ARG at 2^31 - 2 and above; MBPE_ERR_VOCAB at 65,536 and above with
 *                       token_bits 16).  NOT checked: that the mask ends a chunk right before and at the end of every
 *                       single.  That is a precondition; breaking it gives wrong tokens, never a wrong address
 *   doc_off, n_docs     host, optional (NULL / 0): n_docs + 1 ascending byte offsets up to n_bytes, each of them a chunk
 *                       boundary (a precondition as well)
 *   doc_tok_off_out     optional, host, n_docs + 1 entries: [i] = the output tokens that come from the bytes before
 *                       doc_off[i], computed on the device (the rank of doc_off[i] among the mask's end bits, then the
 *                       finishing kernel's list of chunk ends).  Also filled by a query; a cap too small writes [0] only
 *   tokens_out, cap, token_bits, out_on_device, n_out, n_passes_out   as for mbpe_encoder_encode, MBPE_ERR_VOCAB and
 *                       the query included
 * One piece only: a text above the piece limit of mbpe_encoder_encode (option "piece_bytes") returns MBPE_ERR_OOM with
 * a message that names the limit; the encoder stays usable.  A repeat call of no larger size allocates nothing. */
typedef struct { uint64_t start, len; uint32_t id, pad; } mbpe_single;
MBPE_API int  mbpe_encoder_encode_endmask(mbpe_encoder *e, const uint8_t *text_dev, uint64_t n_bytes,
                                          const uint8_t *endmask_dev, const mbpe_single *singles, uint64_t n_singles,
                                          const uint64_t *doc_off, uint64_t n_docs,
                                          void *tokens_out, uint64_t cap, uint32_t token_bits, int out_on_device,
                                          uint64_t *doc_tok_off_out, uint64_t *n_out, uint32_t *n_passes_out);

/* ---- token byte offsets ---------------------------------------------------- */

/* mbpe_encoder_encode and mbpe_encoder_encode_endmask that also say which bytes of `text` every token stands for.  All
 * arguments, results and error codes are those of the counterpart; the one addition:
 *   tok_byte_off_out   optional; lives where tokens_out lives (host memory, or device memory -- 8-byte aligned -- when
 *                      out_on_device != 0) and has room for cap + 1 entries.  On success with *n_out == n it holds
 *                      n + 1 ascending offsets into text: [0] == 0, [n] == n_bytes, and token j stands for
 *                      text[tok_byte_off[j] .. tok_byte_off[j + 1]).  The chunks tile the text and no token crosses a
 *                      chunk, so the tokens tile it too (the convention of chunk_off and chunk_tok_off_out).  A chunk
 *                      that is one token by rule -- NUL-led with a remainder std::stoi parses, or a mbpe_single -- covers
 *                      its whole chunk whatever its id decodes to; an empty chunk contributes nothing.
 *                      NULL: the call IS its counterpart.  Ignored (nothing written) by a query (tokens_out NULL).  A
 *                      cap too small writes no offset.  Pieces: the offsets continue across pieces in 64 bits, the
 *                      result is that of the unsplit call.  Empty text: [0] = 0.
 * Precondition, checked on the host before the device is touched: the encoder's table is one mbpe_merges_check accepts
 * (and no token is longer than 2^32 - 1 bytes).  Only then are the bytes a token covers a function of its id alone:
 * len[256 + k] = len[a_k] + len[b_k].  Any other table: MBPE_ERR_ARG with a message that says so, from these two calls
 * only -- the encoder stays usable and the plain calls take such tables as before.
 * How: after the passes, from the final stream (nothing is carried through the passes; the plain calls run the kernels
 * they ran before): per span of 1,024 tokens a 64-bit byte count, one scan workgroup, a ranked write with a wave prefix
 * sum; the one-token chunks get their chunk's length through a list of their token indices (rank of their start among
 * the mask's end bits -> the finishing kernel's chunk ends).  The new kernels read each token twice and write 8 bytes
 * per token.  Device memory: 4 bytes per token id (len[], uploaded by the first such call and kept), 8 bytes per 1,024
 * text bytes, 8 per one-token chunk and -- only when the offsets go to the host -- a staging buffer of 8 bytes per
 * token of the largest piece.  A piece then costs up to 13.2 + 8 = 21.2 bytes per text byte (every byte its own
 * token), and the limit that "piece_bytes" 0 derives divides by 22 instead of 14 for such a call; with out_on_device it
 * stays 14 (while dropout is on: 30 instead of 22, mbpe_encoder_set_dropout).  A repeat call of no larger size
 * allocates nothing. */
MBPE_API int  mbpe_encoder_encode_byteoff(mbpe_encoder *e, const uint8_t *text, uint64_t n_bytes, int text_on_device,
                                          const uint64_t *chunk_off, uint64_t n_chunks,
                                          void *tokens_out, uint64_t cap, uint32_t token_bits, int out_on_device,
                                          uint64_t *tok_byte_off_out, uint64_t *chunk_tok_off_out, uint64_t *n_out,
                                          uint32_t *n_passes_out);
MBPE_API int  mbpe_encoder_encode_endmask_byteoff(mbpe_encoder *e, const uint8_t *text_dev, uint64_t n_bytes,
                                                  const uint8_t *endmask_dev, const mbpe_single *singles,
                                                  uint64_t n_singles, const uint64_t *doc_off, uint64_t n_docs,
                                                  void *tokens_out, uint64_t cap, uint32_t token_bits, int out_on_device,
                                                  uint64_t *tok_byte_off_out, uint64_t *doc_tok_off_out, uint64_t *n_out,
                                                  uint32_t *n_passes_out);

/* mbpe_encoder_encode_endmask followed by the pack kernel: mbpe_encoder_encode_batch (aux NULL: ids and lengths only) or
 * mbpe_encoder_encode_batch_aux for the documents doc_off describes, which here must start at 0 and end at n_bytes.
 * The documents' token offsets go from the encode to the pack kernel on the device; neither a token nor an offset
 * crosses to the host unless doc_tok_off_out asks for the offsets.  All other arguments and results are those of
 * mbpe_encoder_encode_batch_aux. */
MBPE_API int  mbpe_encoder_encode_batch_endmask(mbpe_encoder *e, const uint8_t *text_dev, uint64_t n_bytes,
                                                const uint8_t *endmask_dev, const mbpe_single *singles,
                                                uint64_t n_singles, const uint64_t *doc_off, uint64_t n_docs,
                                                const mbpe_pack_spec *spec, void *ids_out, uint64_t cap_rows,
                                                int out_on_device, uint32_t *len_out, uint64_t *n_rows_out,
                                                uint64_t *n_tokens_out, const mbpe_pack_aux *aux,
                                                uint64_t *doc_tok_off_out);

/* ---- long documents as overlapping windows --------------------------------- */

/* The third way into [rows, seq_len]: one document per row like MBPE_PACK_PADDED, but a document that does not fit
 * becomes several rows of its own, and consecutive rows share `stride` tokens of context (elsewhere: stride,
 * return_overflowing_tokens, overflow_to_sample_mapping).  With keep = seq_len - nb - ne and step = keep - stride, a
 * document d of L tokens tok[0 .. L) has W_d = 1 windows if L <= keep (an empty one too), else
 * 1 + ceil((L - keep) / step).  Window i holds tok[a .. b), a = i * step, b = min(a + keep, L), and is the last one iff
 * i == W_d - 1; the last window always brings a token no earlier one held.  row_start being the exclusive 64-bit prefix
 * sum of W_d, row row_start[d] + i is [bos] tok[a .. b) [eos] -- bos in every window, eos in the last one only -- then
 * pad_id up to seq_len; len[row] = nb + (b - a) + (ne and last); n_rows = the sum of W_d.  From the same walk
 * (k_pack_windows, csrc/pack.hip):
 *   labels  the bos cell gets tok[a], the cell of tok[t] gets tok[t + 1] -- also across the row end, in a window that
 *           is not the last: the cell of tok[b - 1] gets tok[b] -- and the cell of tok[L - 1] gets eos if it is set,
 *           else ignore_label (the bos cell of an empty document likewise); the eos cell and every pad cell get
 *           ignore_label.  With score_once the bos cell and the first `stride` body cells of every window i >= 1 get
 *           ignore_label too: those targets were labels in window i - 1.  Then, over the rows of one document in
 *           order, the labels that are not ignore_label read tok[0 .. L) with bos (tok[1 .. L) without) and then eos
 *           if it is set: each target exactly once, which is what a sliding-window perplexity sums over
 *   pos     the element's index in its row, 0 .. len - 1; 0 in a pad cell        seg   d + 1; 0 in a pad cell
 *   row_doc [n_rows] the row's document d        row_tok0 [n_rows] a, the index in the document of the row's first
 *           body token; with the token byte offsets of the _byteoff calls, the bytes a row covers
 * When every document has at most keep tokens, ids, len, labels, pos and seg are those of mbpe_pack_tokens_aux with
 * MBPE_PACK_PADDED, bit for bit. */
typedef struct {
    uint32_t  stride;      /* body tokens two consecutive windows of a document share: 0 .. keep - 1 */
    uint32_t  score_once;  /* 0 or 1, see above */
    uint32_t *row_doc;     /* [n_rows] or NULL; on the same side as ids_out */
    uint64_t *row_tok0;    /* [n_rows] or NULL; 8-byte aligned on the device */
} mbpe_pack_window;

/* mbpe_pack_tokens_aux for the window layout.  All arguments up to aux are those of mbpe_pack_tokens_aux; spec->layout
 * must be MBPE_PACK_PADDED with pad_left and trunc_left 0; aux is required, all of its pointers may be NULL.
 * MBPE_ERR_ARG: win NULL, seq_len < nb + ne + 1, stride >= keep, score_once > 1, row_doc with n_docs >= 2^32 - 1, more
 * than 2^40 rows, and the NULL and alignment rules of mbpe_pack_tokens_aux (row_doc 4, row_tok0 8 bytes on the
 * device); MBPE_ERR_VOCAB as for mbpe_pack_tokens.  All of it is checked, and a query (ids_out NULL) answered, on the
 * host before the device is touched; a cap_rows too small is MBPE_ERR_ARG, writes nothing and still reports the count.
 * On the device k_win_rows computes W_d, one scan workgroup and k_win_offsets make row_start of them, then
 * k_pack_windows writes the matrices; mbpe_pack_kernel_ms covers the four.  Device scratch: 8 bytes per document. */
MBPE_API int  mbpe_pack_windows(int device_id, const void *tokens, uint64_t n_tokens, uint32_t token_bits,
                                int tokens_on_device, const uint64_t *doc_tok_off, uint64_t n_docs,
                                const mbpe_pack_spec *spec, void *ids_out, uint64_t cap_rows, int out_on_device,
                                uint32_t *len_out, uint64_t *n_rows_out, const mbpe_pack_aux *aux,
                                const mbpe_pack_window *win);

/* mbpe_encoder_encode_batch_aux and mbpe_encoder_encode_batch_endmask (aux required here too) for the window layout:
 * their arguments, then win.  No token crosses to the host.  The row count depends on the tokens, so it comes back
 * from the device's scan like the token count, and a query (ids_out NULL) runs the passes; a cap_rows too small is
 * found after them, writes nothing and reports the count.  Host outputs, row_doc and row_tok0 included, go through
 * buffers the encoder keeps: a repeat call of no larger size leaves mbpe_encoder_alloc_count as it is.  Windowing
 * happens after the tokens exist, so "rank_order", dropout and "dedup" hold as for the other batch calls.
 * mbpe_encoder_pack_ms covers k_win_rows, the scan, k_win_offsets and k_pack_windows. */
MBPE_API int  mbpe_encoder_encode_batch_windows(mbpe_encoder *e, const uint8_t *text, uint64_t n_bytes,
                                                int text_on_device, const uint64_t *chunk_off, uint64_t n_chunks,
                                                const uint64_t *doc_chunk_off, uint64_t n_docs,
                                                const mbpe_pack_spec *spec, void *ids_out, uint64_t cap_rows,
                                                int out_on_device, uint32_t *len_out, uint64_t *n_rows_out,
                                                uint64_t *n_tokens_out, const mbpe_pack_aux *aux,
                                                uint64_t *doc_tok_off_out, const mbpe_pack_window *win);
MBPE_API int  mbpe_encoder_encode_batch_endmask_windows(mbpe_encoder *e, const uint8_t *text_dev, uint64_t n_bytes,
                                                        const uint8_t *endmask_dev, const mbpe_single *singles,
                                                        uint64_t n_singles, const uint64_t *doc_off, uint64_t n_docs,
                                                        const mbpe_pack_spec *spec, void *ids_out, uint64_t cap_rows,
                                                        int out_on_device, uint32_t *len_out, uint64_t *n_rows_out,
                                                        uint64_t *n_tokens_out, const mbpe_pack_aux *aux,
                                                        uint64_t *doc_tok_off_out, const mbpe_pack_window *win);

/* ---- whole documents packed into rows by best fit -------------------------- */

/* The fourth way into [rows, seq_len]: many whole documents per row, none cut unless it is longer than a row, as little
 * padding as the best-fit-decreasing rule leaves (Ding et al. 2024, "Fewer Truncations Improve Language Modeling").
 * Let S = seq_len.  Document d is the element list E_d = [bos] doc_d [eos] of MBPE_PACK_PACKED, T_d = L_d + nb + ne,
 * never truncated.
 *   Pieces     d has q_d = T_d / S full pieces, piece i holding elements [i * S, (i + 1) * S), and, where
 *              r_d = T_d % S > 0, one tail piece: elements [q_d * S, T_d).  T_d == 0 gives no piece.
 *   Placement  all pieces are taken by size descending, then d ascending, then i ascending.  A piece of size s goes to
 *              the row, among those opened so far with free >= s, that has the smallest free (ties: the lowest row
 *              index), into columns [S - free, S - free + s).  If no row has room a new one is opened -- its index is
 *              the number of rows opened so far -- and the piece starts at column 0.  n_rows = the rows opened.
 * So rows 0 .. F - 1, F = the sum of q_d, are the full pieces in document order; piece sizes do not increase from left
 * to right in a row; padding lies only at the right end of a row and len[row] is the number of cells used; a document
 * with T_d <= S lies in one row, contiguously; at most one row has 2 * len <= S.
 *   Cells      cell (row, col0 + t) of a piece that starts at element k0 of E_d holds element k = k0 + t:
 *              ids E_d[k]; labels E_d[k + 1] if k + 1 < T_d, else ignore_label -- as in PACKED a label crosses a piece
 *              end inside a document and never crosses into another document; pos k, which goes on counting through
 *              the pieces of a long document; seg d + 1.  Pad cells get pad_id, ignore_label, 0 and 0.
 *   doc_row, doc_col   [n_docs]: the cell that holds the first element of the document's last piece (the tail piece if
 *              r_d > 0, else the last full piece); UINT64_MAX and 0 for T_d == 0.  The full pieces of d are the rows
 *              [sum of q_e over e < d, ... + q_d).
 * When every T_d is a multiple of S the matrices are those of mbpe_pack_tokens_aux with MBPE_PACK_PACKED, and when
 * every T_d is one value in (S / 2, S] those with MBPE_PACK_PADDED, bit for bit.
 * Use it only where attention is masked by seg or by cu_seqlens: a row holds unrelated documents. */
struct mbpe_pack_fit {    /* a tag, not a typedef: the call below has the name.  Write `struct mbpe_pack_fit` */
    uint64_t *doc_row;     /* [n_docs] or NULL; on the same side as ids_out, 8-byte aligned on the device */
    uint32_t *doc_col;     /* [n_docs] or NULL; 4-byte aligned on the device */
};

/* The plan alone, on the host (no device, never MBPE_ERR_NO_DEVICE): the row count, the cells used per row and where
 * every document lies.  About O((pieces + rows) * log S) time.
 *   doc_tok_off, n_docs, spec   as for mbpe_pack_fit; out_bits and pad_id play no part
 *   len_out           cap_rows entries, or NULL: count only.  A cap_rows too small is MBPE_ERR_ARG, writes nothing
 *                     and still reports the count
 *   n_rows_out        required
 *   doc_row_out, doc_col_out   optional, n_docs entries each */
MBPE_API int  mbpe_pack_fit_plan(const uint64_t *doc_tok_off, uint64_t n_docs, const mbpe_pack_spec *spec,
                                 uint32_t *len_out, uint64_t cap_rows, uint64_t *n_rows_out, uint64_t *doc_row_out,
                                 uint32_t *doc_col_out);

/* cu_seqlens and max_seqlen of a fit matrix for variable-length attention, on the host alone, with the conventions of
 * mbpe_pack_cu_seqlens (query, cap rule, required outputs).  The list holds the boundaries of the maximal runs of equal
 * (row, seg) in the flattened matrix.  Unlike PACKED, pad runs lie inside the matrix: each counts as a sequence of its
 * own, whose labels are all ignore_label.  The list therefore starts at 0 and ends at n_rows * seq_len (n_rows == 0:
 * [0] and n_seqs 0); max_seqlen is the longest run, pad runs included.  n_rows * seq_len >= 2^31 is MBPE_ERR_ARG. */
MBPE_API int  mbpe_pack_fit_cu_seqlens(const uint64_t *doc_tok_off, uint64_t n_docs, const mbpe_pack_spec *spec,
                                       int32_t *cu_out, uint64_t cap_seqs, uint64_t *n_seqs_out,
                                       uint32_t *max_seqlen_out);

/* mbpe_pack_tokens_aux for the fit layout.  All arguments up to aux are those of mbpe_pack_tokens_aux; spec->layout must
 * be MBPE_PACK_PACKED (so pad_left and trunc_left 0); aux and fit are required, all of their pointers may be NULL.
 * MBPE_ERR_ARG: fit NULL, another layout, more than 2^40 rows, seg with n_docs >= 2^32 - 1, pos with a T_d >= 2^32, and
 * the NULL and alignment rules of mbpe_pack_tokens_aux (doc_row 8, doc_col 4 bytes on the device); MBPE_ERR_VOCAB as for
 * mbpe_pack_tokens.  All of it is checked, the plan made and a query (ids_out NULL: the row count alone) answered on
 * the host before the device is touched; a cap_rows too small is MBPE_ERR_ARG, writes nothing and still reports the
 * count; an error return writes nothing.  The plan is uploaded once per call, 24 bytes per piece and 8 bytes per row
 * of device scratch, and k_pack_fit (csrc/pack.hip) writes the matrices; mbpe_pack_kernel_ms covers it.  doc_row and
 * doc_col are the plan's and are copied to where fit names them. */
MBPE_API int  mbpe_pack_fit(int device_id, const void *tokens, uint64_t n_tokens, uint32_t token_bits,
                            int tokens_on_device, const uint64_t *doc_tok_off, uint64_t n_docs,
                            const mbpe_pack_spec *spec, void *ids_out, uint64_t cap_rows, int out_on_device,
                            uint32_t *len_out, uint64_t *n_rows_out, const mbpe_pack_aux *aux,
                            const struct mbpe_pack_fit *fit);

/* mbpe_encoder_encode_batch_aux and mbpe_encoder_encode_batch_endmask (aux required here too) for the fit layout: their
 * arguments, then fit.  No token crosses to the host.  The documents' token offsets do, after the passes, 8 bytes per
 * document -- the one thing that crosses, also in the endmask call -- because the plan is made on the host; a query
 * (ids_out NULL) therefore runs the passes, and a cap_rows too small is found after them, writes nothing and reports
 * the count.  The plan, its device copy (24 bytes per piece, 8 per row) and the staging of host outputs live in buffers
 * the encoder keeps: a repeat call of no larger size leaves mbpe_encoder_alloc_count as it is.  Packing happens after
 * the tokens exist, so "rank_order", dropout and "dedup" hold as for the other batch calls.  mbpe_encoder_pack_ms
 * covers k_pack_fit. */
MBPE_API int  mbpe_encoder_encode_batch_fit(mbpe_encoder *e, const uint8_t *text, uint64_t n_bytes, int text_on_device,
                                            const uint64_t *chunk_off, uint64_t n_chunks,
                                            const uint64_t *doc_chunk_off, uint64_t n_docs, const mbpe_pack_spec *spec,
                                            void *ids_out, uint64_t cap_rows, int out_on_device, uint32_t *len_out,
                                            uint64_t *n_rows_out, uint64_t *n_tokens_out, const mbpe_pack_aux *aux,
                                            uint64_t *doc_tok_off_out, const struct mbpe_pack_fit *fit);
MBPE_API int  mbpe_encoder_encode_batch_endmask_fit(mbpe_encoder *e, const uint8_t *text_dev, uint64_t n_bytes,
                                                    const uint8_t *endmask_dev, const mbpe_single *singles,
                                                    uint64_t n_singles, const uint64_t *doc_off, uint64_t n_docs,
                                                    const mbpe_pack_spec *spec, void *ids_out, uint64_t cap_rows,
                                                    int out_on_device, uint32_t *len_out, uint64_t *n_rows_out,
                                                    uint64_t *n_tokens_out, const mbpe_pack_aux *aux,
                                                    uint64_t *doc_tok_off_out, const struct mbpe_pack_fit *fit);

/* ---- fill-in-the-middle ---------------------------------------------------- */

/* The fill-in-the-middle transform of token documents (Bavarian et al., 2022: the "FIM rate" and "SPM rate" of code
 * models), between encode and pack: it changes every transformed document's length and therefore every row.  A
 * document is cut at two random points into prefix P, middle M and suffix S and rewritten with three sentinel ids:
 *   PSM   pre P suf S mid M            SPM   pre suf S mid P M
 * For document d of a call let t[0 .. L) be its tokens, g = doc_base + d (mod 2^64) and u_i = h(seed, g, i) for
 * i = 0 .. 3, h the hash of BPE-dropout above (the document number stands where the byte offset stood, the draw's
 * index where the merged id stood).
 *   transformed   iff u_0 < rate, L >= max(min_tokens, 1) and (max_tokens == 0 or L <= max_tokens)
 *   cuts          c1 = (u_1 * (L + 1)) >> 32, c2 = (u_2 * (L + 1)) >> 32 as 64-bit products; a = min(c1, c2),
 *                 b = max(c1, c2), both in [0, L]: P = t[0:a], M = t[a:b], S = t[b:L]; empty parts are allowed
 *   mode          SPM iff u_3 < spm, else PSM; either way the document has L + 3 ids afterwards
 * An untransformed document is copied as it is; an empty one stays empty.  The result is a pure function of (spec, d,
 * L, tokens): the same call gives the same batch, another seed another epoch, and a corpus fed in batches gets the
 * result of one big call by passing in doc_base the number of each batch's first document.  bos and eos stay the
 * packer's business: with eos_id set the end token follows the middle.  Thresholds come from mbpe_dropout_threshold.
 * Tokens are read as the packers read them (16-bit plain ids, or 32-bit with bit 31 ignored) and written as plain
 * ids of the same width.
 * Errors, all before the device is touched: MBPE_ERR_ARG for a threshold above 2^32, max_tokens != 0 with min_tokens >
 * max_tokens, a sentinel id >= 2^31 - 2, a NULL spec where one is required and bad offsets; MBPE_ERR_VOCAB for a
 * sentinel id >= 65,536 with 16-bit tokens; MBPE_ERR_ARG, naming the document, for a document of 2^32 - 1 tokens or
 * more while rate > 0 (where only the device holds the offsets, the plan kernel flags it and the host reads the flag
 * with the new token count). */
typedef struct {
    uint64_t rate;        /* threshold in [0, 2^32]: a document is transformed iff its draw is below it */
    uint64_t spm;         /* threshold in [0, 2^32]: a transformed document is SPM iff its draw is below it, else PSM */
    uint64_t seed;
    uint64_t doc_base;    /* number of the call's first document in the caller's corpus */
    uint32_t pre_id, suf_id, mid_id;
    uint32_t min_tokens;  /* documents shorter than max(min_tokens, 1) stay as they are */
    uint32_t max_tokens;  /* 0: no limit; otherwise documents longer than this stay as they are */
} mbpe_fim_spec;

/* The plan alone, on the host (never MBPE_ERR_NO_DEVICE): doc_tok_off_out (n_docs + 1, required) = the token offsets
 * after the transform; mode_out (n_docs bytes, or NULL) = 0 untransformed / 1 PSM / 2 SPM; cut_out (2 per document,
 * or NULL) = a, b (0, 0 for an untransformed document).  The sentinel ids are checked as for 32-bit tokens. */
MBPE_API int  mbpe_fim_plan(const uint64_t *doc_tok_off, uint64_t n_docs, const mbpe_fim_spec *spec,
                            uint64_t *doc_tok_off_out, uint8_t *mode_out, uint64_t *cut_out);

/* The transform of a flat token stream on HIP device `device_id`, with the conventions of mbpe_pack_tokens: tokens
 * and tokens_out in host or device memory (tokens_on_device / out_on_device; tokens_out on the device aligned to its
 * tokens), doc_tok_off (n_docs + 1) and doc_tok_off_out (n_docs + 1, or NULL) on the host.  *n_out = the new token
 * count.  tokens_out NULL is a query, answered from the host's offsets without a device (doc_tok_off_out is filled);
 * a cap too small is MBPE_ERR_ARG: nothing is written and n_out is still reported.  tokens_out and doc_tok_off_out are
 * what mbpe_pack_* and mbpe_decode_batch take as they are.  Kernels (csrc/fim.hip): k_fim_plan, one lane per document,
 * leaves the plan and the new lengths, a 64-bit scan over spans of 1,024 documents the new offsets; k_fim_gather
 * writes the new stream, a lane per 16-byte piece of it, every token read and written once.  mbpe_fim_kernel_ms: the
 * device time of the calling thread's latest such call. */
MBPE_API int  mbpe_fim_tokens(int device_id, const void *tokens, uint64_t n_tokens, uint32_t token_bits,
                              int tokens_on_device, const uint64_t *doc_tok_off, uint64_t n_docs,
                              const mbpe_fim_spec *spec, void *tokens_out, uint64_t cap, int out_on_device,
                              uint64_t *doc_tok_off_out, uint64_t *n_out);
MBPE_API int  mbpe_fim_kernel_ms(float *ms_out);

/* The transform as a stage of the encoder's batch calls; spec NULL turns it off.  It holds from the next call on for
 * every call that packs: mbpe_encoder_encode_batch, _aux, _windows, _fit and the four _endmask batch calls.  The stage
 * runs between the encode and the pack kernel, into a second flat buffer and offset array the encoder keeps (a repeat
 * call of no larger size leaves mbpe_encoder_alloc_count as it is); everything downstream -- the rows, the window and
 * fit plans, labels, pos and seg -- sees the transformed documents.  doc_tok_off_out gives the offsets AFTER the
 * transform: what the matrices were built from and what the cu_seqlens calls take.  n_tokens_out stays "tokens
 * encoded", so doc_tok_off_out[n_docs] == n_tokens_out + 3 * (documents transformed).  The sentinel ids are checked
 * against the width of the tokens a call packs from (16 bits with out_bits 16) when the call is made.  The flat encode
 * calls, the count calls and mbpe_encode_chunks* are unaffected.  Dropout and "dedup" combine freely: they act before
 * the stage.  With no spec, and with rate 0, every call launches and allocates exactly what it does without.
 * mbpe_encoder_kernel_ms and mbpe_encoder_pack_ms include the stage.
 * mbpe_encoder_fim_info: the plan of the latest batch call, on the host: *n_docs_out = its documents; mode_out
 * (bytes) and cut_out (2 per document), each NULL or with room for cap_docs documents (fewer than n_docs:
 * MBPE_ERR_ARG, the count is still reported).  All zero where the stage was off. */
MBPE_API int  mbpe_encoder_set_fim(mbpe_encoder *e, const mbpe_fim_spec *spec);
MBPE_API int  mbpe_encoder_fim_info(mbpe_encoder *e, uint8_t *mode_out, uint64_t *cut_out, uint64_t cap_docs,
                                    uint64_t *n_docs_out);

/* ---- masked-LM batches ----------------------------------------------------- */

/* Masked-LM corruption of token documents (Devlin et al., 2019: select 15 % of the tokens, replace 80 % of those by a
 * mask id, 10 % by a random id, leave 10 % as they are), between encode and pack, token by token or -- whole_word -- word
 * by word, a word being a chunk of the encoder's split: in a 32-bit device stream bit 31 of a token says "last token of
 * its word", and a document's last token ends a word whether flagged or not.  For document d of a call let t[0 .. L) be
 * its tokens, g = doc_base + d (mod 2^64), h the hash of BPE-dropout above and
 *   s_g = (h(seed, g, 0x4D4C4D00) << 32) | h(seed, g, 0x4D4C4D01).
 * Token k belongs to the word whose first token has index w(k): w(k) = k if k == 0, or whole_word == 0, or token k - 1
 * is flagged; otherwise w(k) = w(k - 1).
 *   selected      iff h(s_g, w(k), 0) < select and the token's id is not among protect[0 .. n_protect)
 *   replacement   for a selected token r = h(s_g, k, 1): r < mask gives mask_id; else r < mask + random gives
 *                 (h(s_g, k, 2) * vocab_n) >> 32 as a 64-bit product, an id in [0, vocab_n); else the id stays
 *   target        target[k] = the old id if the token is selected, else MBPE_NO_TOKEN
 * The new stream has the length of the old one, so doc_tok_off holds for both; it is written as plain ids of the
 * input's width.  The target stream is uint32 whatever the width.  The result is a pure function of (spec, d, tokens
 * of d): the same call gives the same batch, another seed another epoch, a corpus fed in batches gets the result of one
 * big call by passing in doc_base the number of each batch's first document, and a document is masked alike in every
 * layout it is packed into.  Thresholds come from mbpe_dropout_threshold.  A protected token inside a selected word
 * stays and is no target; the rest of the word is masked.  Random ids are drawn from all of [0, vocab_n): special ids
 * below vocab_n included.
 * Errors, all before the device is touched: MBPE_ERR_ARG for a threshold above 2^32, mask + random > 2^32, random > 0
 * with vocab_n == 0, n_protect > 8, whole_word > 1, mask_id or vocab_n >= 2^31 - 2, whole_word with 16-bit tokens (they
 * carry no flag), bad offsets and a NULL spec where one is required; MBPE_ERR_VOCAB for mask_id >= 65,536 or
 * vocab_n > 65,536 with 16-bit tokens. */
typedef struct {
    uint64_t select;      /* threshold in [0, 2^32]: a word (a token without whole_word) is selected iff its draw is below it */
    uint64_t mask;        /* threshold in [0, 2^32]: a selected token becomes mask_id iff its draw is below it */
    uint64_t random;      /* threshold in [0, 2^32 - mask]: the share next to it becomes a random id */
    uint64_t seed;
    uint64_t doc_base;    /* number of the call's first document in the caller's corpus */
    uint32_t mask_id;
    uint32_t vocab_n;     /* random ids are drawn from [0, vocab_n) */
    uint32_t whole_word;  /* 0 or 1 */
    uint32_t n_protect;   /* ids of protect[] in use: 0 .. 8 */
    uint32_t protect[8];  /* ids that are never selected (bos, eos, separators) */
} mbpe_mlm_spec;

/* The rule on the host alone (never MBPE_ERR_NO_DEVICE): tokens (n_tokens of token_bits bits, host memory; 32-bit
 * tokens with bit 31 = word end) and doc_tok_off (n_docs + 1) -> tokens_out (n_tokens plain ids of token_bits bits, or
 * NULL) and targets_out (n_tokens uint32, or NULL). */
MBPE_API int  mbpe_mlm_plan(const void *tokens, uint64_t n_tokens, uint32_t token_bits, const uint64_t *doc_tok_off,
                            uint64_t n_docs, const mbpe_mlm_spec *spec, void *tokens_out, uint32_t *targets_out);

/* The same of a flat token stream on HIP device `device_id`, with the conventions of mbpe_fim_tokens: tokens in host
 * or device memory (tokens_on_device), tokens_out (required, n_tokens ids) and targets_out (n_tokens uint32, or NULL)
 * both in host or both in device memory (out_on_device; on the device aligned to their elements), doc_tok_off on the
 * host.  There is no query form: the length does not change.  n_tokens == 0 is no device call.  The outputs are what
 * mbpe_pack_tokens_aux_labels, mbpe_pack_windows_labels and mbpe_pack_fit_labels take as tokens and label_tokens.
 * Kernels (csrc/mlm.hip): k_mlm_apply, a lane per 16 bytes of tokens, reads every token once and writes the new id and
 * the target once, all in 16-byte pieces where the three addresses are 16-byte aligned (id by id otherwise); a lane
 * finds its document by one search per span of 1,024 tokens.  With whole_word k_mlm_starts first leaves the latest
 * word start of every span and k_mlm_scan the running maximum over the spans, which k_mlm_apply carries on.
 * mbpe_mlm_kernel_ms: the device time of the calling thread's latest such call. */
MBPE_API int  mbpe_mlm_tokens(int device_id, const void *tokens, uint64_t n_tokens, uint32_t token_bits,
                              int tokens_on_device, const uint64_t *doc_tok_off, uint64_t n_docs,
                              const mbpe_mlm_spec *spec, void *tokens_out, uint32_t *targets_out, int out_on_device);
MBPE_API int  mbpe_mlm_kernel_ms(float *ms_out);

/* mbpe_pack_tokens_aux, mbpe_pack_windows and mbpe_pack_fit with the labels taken from a target stream instead of the
 * next token: each is the call it is named after plus label_tokens, n_tokens uint32 on the same side as tokens
 * (required: NULL is MBPE_ERR_ARG; 4-byte aligned on the device).  A cell that holds body token j of the stream gets
 * label_tokens[j], or ignore_label where that is MBPE_NO_TOKEN; bos, eos and pad cells get ignore_label.  In windows
 * with score_once the cells a window shares with the one before it get ignore_label as they do without, so a token is
 * a target at most once.  ids, len, pos, seg and every other output are untouched.  With out_bits 16 a label is the
 * low 16 bits of its entry. */
MBPE_API int  mbpe_pack_tokens_aux_labels(int device_id, const void *tokens, uint64_t n_tokens, uint32_t token_bits,
                                          int tokens_on_device, const uint64_t *doc_tok_off, uint64_t n_docs,
                                          const mbpe_pack_spec *spec, void *ids_out, uint64_t cap_rows,
                                          int out_on_device, uint32_t *len_out, uint64_t *n_rows_out,
                                          const mbpe_pack_aux *aux, const uint32_t *label_tokens);
MBPE_API int  mbpe_pack_windows_labels(int device_id, const void *tokens, uint64_t n_tokens, uint32_t token_bits,
                                       int tokens_on_device, const uint64_t *doc_tok_off, uint64_t n_docs,
                                       const mbpe_pack_spec *spec, void *ids_out, uint64_t cap_rows, int out_on_device,
                                       uint32_t *len_out, uint64_t *n_rows_out, const mbpe_pack_aux *aux,
                                       const mbpe_pack_window *win, const uint32_t *label_tokens);
MBPE_API int  mbpe_pack_fit_labels(int device_id, const void *tokens, uint64_t n_tokens, uint32_t token_bits,
                                   int tokens_on_device, const uint64_t *doc_tok_off, uint64_t n_docs,
                                   const mbpe_pack_spec *spec, void *ids_out, uint64_t cap_rows, int out_on_device,
                                   uint32_t *len_out, uint64_t *n_rows_out, const mbpe_pack_aux *aux,
                                   const struct mbpe_pack_fit *fit, const uint32_t *label_tokens);

/* The corruption as a stage of the encoder's batch calls; spec NULL turns it off.  It holds from the next call on for
 * every call that packs (those of mbpe_encoder_set_fim).  The stage runs after the encode -- so after dropout and
 * "dedup" -- and before the pack kernel, into a second flat buffer and a target buffer the encoder keeps (a repeat call
 * of no larger size leaves mbpe_encoder_alloc_count as it is); the matrices hold the new ids, and labels -- where aux
 * asks for them -- the targets as in the _labels calls above.  The plain batch calls without aux get the new ids alone.
 * Both stages on is MBPE_ERR_ARG from the batch call, never a silent choice.  whole_word reads the flagged 32-bit
 * stream the passes leave, which every route keeps up to the stage (host split, endmask, both orders, dropout, "dedup",
 * texts cut into pieces, one-token chunks); with out_bits 16 the flat stream is 16 bits wide and whole_word is
 * MBPE_ERR_ARG from the batch call, as are a mask_id or vocab_n that do not fit (MBPE_ERR_VOCAB).  With no spec, and
 * with select 0, every call launches and allocates exactly what it does without.  mbpe_encoder_kernel_ms and
 * mbpe_encoder_pack_ms include the stage. */
MBPE_API int  mbpe_encoder_set_mlm(mbpe_encoder *e, const mbpe_mlm_spec *spec);

/* ---- span-corruption (denoise) batches for encoder-decoder models ------------ */

/* T5 / UL2-style span corruption (Raffel et al., 2020) between encode and pack: runs of tokens are replaced by sentinel
 * ids in the INPUTS, and the dropped runs follow their sentinels in the TARGETS.  One stream becomes two, and a long
 * document becomes several units first (T5's split_tokens), so the stage also changes the number of rows.  ("Span"
 * already means 1,024 scan elements in this code base, hence the name.)  All of it is integer arithmetic; h is the hash
 * of BPE-dropout above.
 *   units       document d of the call has L_d tokens and g = doc_base + d (mod 2^64).  It has U_d = 1 units if
 *               segment_tokens == 0, else max(1, ceil(L_d / segment_tokens)); an empty document keeps one empty unit.
 *               Unit u holds the tokens [u * seg, min((u + 1) * seg, L_d)); units are numbered through the call in
 *               document order
 *   seeds       s_g = (h(seed, g, 0x44454E00) << 32) | h(seed, g, 0x44454E01);  s_u = (h(s_g, u, 2) << 32) | h(s_g, u, 3)
 *   counts      a unit of L tokens stays as it is (inputs = its tokens, no targets) if density == 0 or
 *               L < max(min_tokens, 2).  Otherwise N = clamp((L * density + 2^31) >> 32, 1, L - 1) tokens are noise, in
 *               S = clamp((N * 256 + mean_span_q8 / 2) / mean_span_q8, 1, min(N, L - N, n_sentinels)) parts
 *   boundaries  to cut a total T into S parts >= 1 with draw c: E = T - S, q(j) = floor(j * E / S), c_0 = 0, c_S = E,
 *               c_j = q(j - 1) + ((h(s_u, j, c) * (q(j) - q(j - 1) + 1)) >> 32) for 0 < j < S, and B_j = j + c_j.
 *               Every cut lies in its own stratum, so B ascends strictly and any B_j costs one hash.
 *               Bn = boundaries(N, S, 0) are the noise parts, Bm = boundaries(L - N, S, 1) the kept parts
 *   layout      kept part 0, noise part 0, kept part 1, .. noise part S - 1, with s_j the sentinel of part j
 *               (sentinel_id - j with sentinel_down, T5's <extra_id_j>; else sentinel_id + j):
 *                 inputs  = kept_0 s_0 kept_1 s_1 .. kept_{S-1} s_{S-1}        L - N + S ids
 *                 targets = s_0 noise_0 s_1 noise_1 .. s_{S-1} noise_{S-1}     N + S ids
 * The result is a pure function of (spec, d, tokens of d): the same call gives the same batch, another seed another
 * epoch, and a corpus fed in batches gets the result of one big call by passing in doc_base the number of each batch's
 * first document.  Thresholds come from mbpe_dropout_threshold.  Tokens are read as the packers read them (16-bit plain
 * ids, or 32-bit with bit 31 ignored) and written as plain ids of the same width.  eos and the decoder start id stay
 * the packer's business.
 * Errors, all before the device is touched: MBPE_ERR_ARG for a NULL spec where one is required, density > 2^32,
 * mean_span_q8 < 256, n_sentinels == 0, sentinel_down > 1, a sentinel range that leaves [0, 2^31 - 2), bad offsets,
 * more than 2^40 units or ids, and -- naming the document -- a unit of 2^32 - 1 tokens or more while density > 0 (where
 * only the device holds the offsets, a flag word is read back with the totals); MBPE_ERR_VOCAB for a sentinel
 * >= 65,536 with 16-bit tokens. */
typedef struct {
    uint64_t density;        /* threshold in [0, 2^32]: share of a unit's tokens that become noise (T5: 0.15) */
    uint64_t seed;
    uint64_t doc_base;       /* number of the call's first document in the caller's corpus */
    uint32_t mean_span_q8;   /* mean noise-part length in 1/256 tokens, >= 256 (T5: 3.0 = 768) */
    uint32_t segment_tokens; /* 0: a document is one unit; else it is cut into units of this many tokens, the last shorter */
    uint32_t min_tokens;     /* units shorter than max(min_tokens, 2) stay as they are */
    uint32_t sentinel_id;    /* id of part 0's sentinel */
    uint32_t sentinel_down;  /* 1: part j gets sentinel_id - j (T5's <extra_id_j>), 0: sentinel_id + j */
    uint32_t n_sentinels;    /* >= 1: no unit gets more parts than this */
} mbpe_denoise_spec;         /* 48 bytes; sentinel_id at offset 36 */

/* The plan alone, on the host (never MBPE_ERR_NO_DEVICE): *n_units_out (required) = the units of the call;
 * unit_in_off and unit_tg_off (n_units + 1 each) = the units' offsets into the inputs and into the targets;
 * unit_doc (n_units) = each unit's document.  Each of the three is NULL or has room for cap_units units; a cap too
 * small is MBPE_ERR_ARG, writes nothing and still reports the count.  The sentinels are checked as for 32-bit tokens. */
MBPE_API int  mbpe_denoise_plan(const uint64_t *doc_tok_off, uint64_t n_docs, const mbpe_denoise_spec *spec,
                                uint64_t *n_units_out, uint64_t *unit_in_off, uint64_t *unit_tg_off, uint64_t *unit_doc,
                                uint64_t cap_units);

/* The two streams of a flat token stream on HIP device `device_id`, with the conventions of mbpe_fim_tokens: tokens in
 * host or device memory (tokens_on_device), doc_tok_off (n_docs + 1) on the host; inputs_out (cap_in ids) and
 * targets_out (cap_tg ids) both in host or both in device memory (out_on_device; on the device aligned to their ids);
 * the three unit arrays of mbpe_denoise_plan on the host, each NULL or with room for cap_units.  n_units_out, n_in_out
 * and n_tg_out are required.  inputs_out NULL is a query, answered from the host's plan without a device (the unit
 * arrays are filled); a cap too small -- cap_in, cap_tg or, with a unit array given, cap_units -- is MBPE_ERR_ARG: nothing
 * is written and the counts are still reported.  (inputs_out, unit_in_off) and (targets_out, unit_tg_off) are what
 * mbpe_pack_tokens* and mbpe_decode_batch take as they are, one row per unit.
 * Kernels (csrc/denoise.hip): k_dn_units, one lane per document, and a 64-bit scan over spans of 1,024 documents leave
 * the unit offsets; k_dn_lengths, one lane per unit, finds its document by binary search and leaves both lengths, two
 * scans the two offset arrays; k_dn_gather runs once per side, a lane per 16-byte piece of the output: it finds its
 * unit and its part by binary search (one hash per probe) and walks, every token read once and written once.  No table
 * of part boundaries is ever stored.  With ids asked for, the unit arrays handed back are the device's own.
 * mbpe_denoise_kernel_ms: the device time of the calling thread's latest such call. */
MBPE_API int  mbpe_denoise_tokens(int device_id, const void *tokens, uint64_t n_tokens, uint32_t token_bits,
                                  int tokens_on_device, const uint64_t *doc_tok_off, uint64_t n_docs,
                                  const mbpe_denoise_spec *spec, void *inputs_out, uint64_t cap_in, void *targets_out,
                                  uint64_t cap_tg, int out_on_device, uint64_t *unit_in_off, uint64_t *unit_tg_off,
                                  uint64_t *unit_doc, uint64_t cap_units, uint64_t *n_units_out, uint64_t *n_in_out,
                                  uint64_t *n_tg_out);
MBPE_API int  mbpe_denoise_kernel_ms(float *ms_out);

/* What the two batch calls below write, one row per unit; on the same side as each other (out_on_device), on the device
 * dec_ids and dec_labels 16-byte aligned, the others aligned to their elements.
 *   enc_ids     [rows, enc_spec->seq_len] ids: the inputs packed with enc_spec.  NULL: query
 *   enc_len     [rows] or NULL
 *   dec_ids     [rows, dec_spec->seq_len] ids: the targets packed with dec_spec through the aux packer.  Required with
 *               enc_ids.  With dec_spec->bos_id = the decoder start id and eos_id set, dec_ids / dec_labels are T5's
 *               decoder_input_ids / labels
 *   dec_len     [rows] or NULL
 *   dec_labels  [rows, dec_spec->seq_len] ids or NULL: next-token labels of dec_ids, ignore_label elsewhere
 *   row_doc     [rows] or NULL: the row's document */
typedef struct {
    void     *enc_ids;
    uint32_t *enc_len;
    void     *dec_ids;
    uint32_t *dec_len;
    void     *dec_labels;
    uint32_t *row_doc;
    int64_t   ignore_label;
} mbpe_denoise_batch;

/* Encode, the stage, then two PADDED packs with the pack kernels on the encoder's stream: mbpe_encoder_encode_batch_aux
 * and mbpe_encoder_encode_batch_endmask for encoder-decoder batches.  Arguments up to n_docs as for those calls; dn the
 * rule's spec; enc_spec and dec_spec the two matrices' specs, both MBPE_PACK_PADDED with equal out_bits (anything else
 * is MBPE_ERR_ARG); out as above with room for cap_rows rows.  No token crosses to the host.  *n_rows_out = the units
 * of the call: it comes back from the device, so a query (out->enc_ids NULL) runs the passes and the unit and length
 * kernels, and a cap_rows too small is found after them, writes nothing and reports the count.  n_tokens_out stays
 * "tokens encoded".  Buffers are kept by the encoder: a repeat call of no larger size leaves mbpe_encoder_alloc_count
 * as it is.  mbpe_encoder_kernel_ms and mbpe_encoder_pack_ms include the stage.  "rank_order", dropout and "dedup" act
 * before the stage and combine freely.  mbpe_encoder_set_fim and mbpe_encoder_set_mlm do not apply here: a call while
 * either is on is MBPE_ERR_ARG, never a silent choice.  The sentinels are checked against the width of the tokens the
 * call packs from (16 bits with out_bits 16: MBPE_ERR_VOCAB).  row_doc needs n_docs < 2^32 - 1. */
MBPE_API int  mbpe_encoder_encode_batch_denoise(mbpe_encoder *e, const uint8_t *text, uint64_t n_bytes, int text_on_device,
                                                const uint64_t *chunk_off, uint64_t n_chunks,
                                                const uint64_t *doc_chunk_off, uint64_t n_docs,
                                                const mbpe_denoise_spec *dn, const mbpe_pack_spec *enc_spec,
                                                const mbpe_pack_spec *dec_spec, const mbpe_denoise_batch *out,
                                                uint64_t cap_rows, int out_on_device, uint64_t *n_rows_out,
                                                uint64_t *n_tokens_out);
MBPE_API int  mbpe_encoder_encode_batch_endmask_denoise(mbpe_encoder *e, const uint8_t *text_dev, uint64_t n_bytes,
                                                        const uint8_t *endmask_dev, const mbpe_single *singles,
                                                        uint64_t n_singles, const uint64_t *doc_off, uint64_t n_docs,
                                                        const mbpe_denoise_spec *dn, const mbpe_pack_spec *enc_spec,
                                                        const mbpe_pack_spec *dec_spec, const mbpe_denoise_batch *out,
                                                        uint64_t cap_rows, int out_on_device, uint64_t *n_rows_out,
                                                        uint64_t *n_tokens_out);

/* ---- decode on the device ----------------------------------------------- */

/* Tokenizer::decode (Tokenizer.h:725-751) for whole token streams on HIP device `device_id`: per token a byte
 * length, a 64-bit exclusive prefix sum, a copy of every token's bytes to its offset (csrc/decode.hip).  What a
 * token id yields, in the reference's order:
 *   - an id among special_ids: that special's bytes.  This test comes first: a special whose id lies below the
 *     vocabulary size overrides the vocabulary entry (:729-733); of several specials with one id the last holds
 *   - otherwise an id >= 256 + n_merges: nothing (the reference prints a warning and goes on, :734-737); such ids
 *     are counted in n_invalid_out
 *   - otherwise vocab[id], with vocab[256 + k] = vocab[a_k] ++ vocab[b_k] (:562-564), a repeated pair included.  A
 *     side of merge k that names an id >= 256 + k contributes nothing, as in the host Tokenizer's rebuilt vocabulary
 *     of a hand-edited model: device and host decode agree on every model the host accepts.
 * A decoder holds, on the device, one length and one offset per id and the bytes of all entries in one blob.  The
 * blob may hold up to MBPE_DECODER_MAX_BLOB bytes and a single entry up to MBPE_DECODER_MAX_ENTRY bytes (so that
 * the 1,024 tokens one wave expands stay below 2^32 bytes); a vocabulary beyond either returns MBPE_ERR_OOM.
 *   merges            2 * n_merges u32, as for mbpe_encode_chunks; n_merges <= MBPE_MAX_VOCAB_WIDE - 256
 *   special_ids       n_special ids; special k's bytes are special_bytes[special_off[k] .. special_off[k+1])
 *                     (special_off: n_special + 1 ascending offsets; an empty string is allowed)
 * Arguments are checked, and the vocabulary is built, before the device is touched.  No CPU fallback:
 * MBPE_ERR_NO_DEVICE without a HIP device.  A decoder has its own non-blocking stream and is thread-compatible
 * like a context: one call at a time. */
#define MBPE_DECODER_MAX_BLOB  (1ull << 30)
#define MBPE_DECODER_MAX_ENTRY ((1u << 22) - 1u)
typedef struct mbpe_decoder mbpe_decoder;
MBPE_API int  mbpe_decoder_create(int device_id, const uint32_t *merges, uint32_t n_merges,
                                  const uint32_t *special_ids, const uint8_t *special_bytes,
                                  const uint64_t *special_off, uint32_t n_special, mbpe_decoder **out);
MBPE_API void mbpe_decoder_destroy(mbpe_decoder *d);

/* Decodes n_tokens ids.  tokens / bytes_out are host memory, or device memory of the decoder's device when
 * tokens_on_device / out_on_device is set (device buffers are used in place: no copy).  bytes_out NULL: query.
 * n_out always receives the decoded length; when cap is smaller the call returns MBPE_ERR_ARG and writes nothing.
 * n_invalid_out (optional): ids that decoded to nothing.  Lengths and offsets are 64-bit throughout: an output
 * beyond 4 GiB is a supported case. */
MBPE_API int  mbpe_decode_tokens(mbpe_decoder *d, const uint32_t *tokens, uint64_t n_tokens, int tokens_on_device,
                                 uint8_t *bytes_out, uint64_t cap, int out_on_device,
                                 uint64_t *n_out, uint64_t *n_invalid_out);

/* The same for a batch of n_docs documents, a document being any run of consecutive tokens (a text of an encoded
 * batch, a chunk, a line), with the byte offset of every document boundary: ONE device call instead of one per
 * document.
 *   tokens            n_tokens ids of token_bits bits, host or device memory (tokens_on_device).  token_bits 32:
 *                     uint32_t ids, read as mbpe_decode_tokens reads them.  token_bits 16: plain uint16_t ids with no
 *                     flag and no hole value, as mbpe_encoder_encode writes them with token_bits 16 -- id 65,535 is a
 *                     token like any other (in the 16-bit layouts of mbpe_decode_slots 0xFFFF stays a hole).  Any
 *                     other token_bits is MBPE_ERR_ARG.
 *   doc_tok_off       host, n_docs + 1 ascending offsets with [0] == 0 and [n_docs] == n_tokens: document i is tokens
 *                     [doc_tok_off[i], doc_tok_off[i + 1]), equal neighbours are an empty document.  The convention of
 *                     chunk_off (mbpe_load_corpus) and of chunk_tok_off_out (mbpe_encoder_encode), whose arrays can be
 *                     passed as they are.  Anything else is MBPE_ERR_ARG before the device is touched; n_docs == 0
 *                     goes with n_tokens == 0 only.
 *   bytes_out, cap, out_on_device, n_out, n_invalid_out   as for mbpe_decode_tokens: the documents' texts one after
 *                     the other, the bytes mbpe_decode_tokens gives for the same tokens
 *   doc_byte_off_out  required; host, n_docs + 1 entries: [b] = the bytes that tokens [0, doc_tok_off[b]) decode to.
 *                     [0] == 0, [n_docs] == *n_out, document i's text is bytes_out[doc_byte_off_out[i] ..
 *                     doc_byte_off_out[i + 1]).  Filled whenever the lengths were computed: also by a query and when
 *                     cap is too small, so that buffers can be sized from them.
 * The limits are those of mbpe_decode_tokens.  The decoder keeps the device copies of both offset arrays between
 * calls like its other scratch: a repeat call of no larger size allocates nothing. */
MBPE_API int  mbpe_decode_batch(mbpe_decoder *d, const void *tokens, uint64_t n_tokens, uint32_t token_bits,
                                int tokens_on_device, const uint64_t *doc_tok_off, uint64_t n_docs,
                                uint8_t *bytes_out, uint64_t cap, int out_on_device,
                                uint64_t *doc_byte_off_out, uint64_t *n_out, uint64_t *n_invalid_out);

/* The same for n_slots device-resident slots in one of the layouts mbpe_stream_device describes (slot_bits 16 or
 * 32, its end_bit and barrier values; an all-ones slot and a barrier slot yield nothing and are not invalid), and
 * for the 32-bit tokens with bit 31 = chunk end that mbpe_encode_chunks_device leaves on the device. */
MBPE_API int  mbpe_decode_slots(mbpe_decoder *d, const void *slots, uint64_t n_slots, uint32_t slot_bits,
                                uint32_t end_bit, uint32_t barrier, uint8_t *bytes_out, uint64_t cap,
                                int out_on_device, uint64_t *n_out, uint64_t *n_invalid_out);

/* Device time of the decoder's latest call in milliseconds (HIP events on its stream around the length kernel, the
 * scan, a batch's boundary-offset kernel and the copy kernel; host <-> device copies are outside). */
MBPE_API int  mbpe_decoder_kernel_ms(const mbpe_decoder *d, float *ms_out);

/* Device allocations (hipMalloc calls) the decoder has made since it was created, its tables included.  A call of
 * no larger size than an earlier one (tokens, documents, output) leaves the number as it is. */
MBPE_API int  mbpe_decoder_alloc_count(const mbpe_decoder *d, uint64_t *n_out);

/* The live stream of a training context, expanded with that training's own merges so far (after
 * mbpe_train_begin; any slot layout, and the 32-bit continuation): decode(stream) == the corpus the context
 * trains on (the packed chunks of a corpus given as ranges; on a rank of a sharded training, that rank's shard).
 * Same conventions for bytes_out / cap / n_out as mbpe_decode_tokens. */
MBPE_API int  mbpe_decode_stream(mbpe_ctx *ctx, uint8_t *bytes_out, uint64_t cap, int out_on_device, uint64_t *n_out);

/* ---- multi-GPU (one process per GPU, RCCL over xGMI) ---------------- */

/* Rank 0 creates the id, every rank receives it out of band (the launcher
 * broadcasts it, e.g. over torch.distributed) and calls mbpe_comm_init.
 * After that mbpe_load_corpus takes the rank's contiguous shard of the
 * corpus (whole chunks for chunked corpora; any byte range of a one-chunk
 * corpus) and training all-reduces the per-merge count deltas and boundary
 * descriptors so every rank takes identical decisions. */
#define MBPE_COMM_ID_BYTES 128
MBPE_API int mbpe_comm_unique_id(uint8_t id_out[MBPE_COMM_ID_BYTES]);
MBPE_API int mbpe_comm_init(mbpe_ctx *ctx, const uint8_t id[MBPE_COMM_ID_BYTES],
                            int rank, int n_ranks);

/* The same sharded algorithm with the collective left to the caller (any
 * transport that can sum u32 buffers across ranks: MPI, gloo, a test harness).
 * After mbpe_comm_init_external, mbpe_train_begin and mbpe_train_steps return
 * MBPE_NEED_EXCHANGE each time the ranks have to exchange data: the caller
 * sum-all-reduces the buffer named by mbpe_comm_exchange_buffer (device
 * memory, u32 elements, identical length on every rank) in place and calls
 * mbpe_comm_exchange_done, which continues the operation and returns
 * MBPE_NEED_EXCHANGE again (next merge) or MBPE_OK (operation complete). */
MBPE_API int mbpe_comm_init_external(mbpe_ctx *ctx, int rank, int n_ranks);
MBPE_API int mbpe_comm_exchange_buffer(mbpe_ctx *ctx, void **dev_ptr_out, uint64_t *n_u32_out);
MBPE_API int mbpe_comm_exchange_done(mbpe_ctx *ctx);

/* ---- host-side pieces of the reference path ------------------------- */

/* Regex pre-split, Tokenizer.h:500-540: successive non-empty PCRE2 matches
 * (options PCRE2_UTF|PCRE2_UCP, +PCRE2_CASELESS when the pattern contains
 * "(?i:", :407-415; PCRE2_NO_UTF_CHECK at match time, :512) become chunks
 * [starts[c], ends[c]).  Bytes between matches belong to no chunk: the reference skips them
 * (:506-540; the built-in gpt2/gpt4 patterns leave none on valid UTF-8).  When the chunks tile
 * the text, mbpe_split_offsets gives the n_chunks + 1 offsets mbpe_load_corpus takes; otherwise it
 * returns NULL and the chunks go to mbpe_load_corpus_ranges. */
typedef struct mbpe_split mbpe_split;
MBPE_API int  mbpe_presplit(const char *pattern, const uint8_t *text, uint64_t n_bytes,
                            mbpe_split **out);
MBPE_API uint64_t        mbpe_split_count(const mbpe_split *s);
MBPE_API const uint64_t *mbpe_split_offsets(const mbpe_split *s);
MBPE_API int             mbpe_split_has_gaps(const mbpe_split *s);
MBPE_API const uint64_t *mbpe_split_starts(const mbpe_split *s);
MBPE_API const uint64_t *mbpe_split_ends(const mbpe_split *s);
MBPE_API void            mbpe_split_free(mbpe_split *s);

/* The split patterns of Tokenizer.h:59-60 ("gpt2", "gpt4"; "basic" = ""). */
MBPE_API const char *mbpe_split_pattern(const char *encoder_name);

/* What PCRE2 (the library and the options mbpe_presplit uses: PCRE2_UTF | PCRE2_UCP) says of every code point
 * 0 .. 0x10FFFF, asked of it once per process on the first call:
 *   cls_out       optional, 0x110000 / 16 words: 2 bits per code point, bits 2 * (cp & 15) and up of word cp >> 4:
 *                 0 = \p{L}, 1 = \p{N}, 2 = \s, 3 = none of them (the surrogates read 3)
 *   fold_cp_out, fold_to_out, cap_fold   optional: the code points >= 0x80 that match one of the letters
 *                 s d m t l v e r under PCRE2_CASELESS (the gpt4 contractions), ascending, each with that letter
 *   n_fold_out    optional: how many there are (MBPE_ERR_ARG when cap_fold is smaller and an array is given)
 *   build_ms_out  optional: what building the table took, in milliseconds
 * MBPE_ERR_REGEX when the library is missing or disagrees with the byte rule below 0x80. */
MBPE_API int mbpe_split_unicode_table(uint32_t *cls_out, uint32_t *fold_cp_out, uint8_t *fold_to_out, uint32_t cap_fold,
                                      uint32_t *n_fold_out, double *build_ms_out);

/* ---- the gpt2 / gpt4 pre-split on the device ------------------------------ */

/* A splitter: mbpe_presplit for the two built-in patterns as an object on HIP device `device_id` (csrc/split.hip,
 * DESIGN.md 4g).  The device decides what ASCII bytes decide: a position where a letter or digit is followed by
 * whitespace is a chunk boundary under either pattern, and a stretch between two such positions that holds only
 * ASCII and is at most "max_span" bytes long is split by a rule on byte classes (csrc/split_rule.h).  Every other
 * stretch -- a "host span" -- is matched by PCRE2 on the host exactly as mbpe_presplit would match it, and its chunk
 * ends are added to the mask on the device.  The result is the split of mbpe_presplit, chunk for chunk.
 *   pattern   byte-equal to mbpe_split_pattern("gpt2") or ("gpt4"); anything else is MBPE_ERR_ARG
 * Arguments are checked before the device is touched.  No CPU fallback: MBPE_ERR_NO_DEVICE without a HIP device.
 * A splitter has its own non-blocking stream and is thread-compatible like a context: one call at a time. */
#define MBPE_SPLIT_BLOCK    64u    /* text bytes per thread of the walk; the sync pass takes 16 per lane */
#define MBPE_SPLIT_TILE     16384u /* text bytes per workgroup of the walk (256 threads) */
#define MBPE_SPLIT_MAX_SPAN 4096u  /* default of the option "max_span" */
typedef struct mbpe_splitter mbpe_splitter;
MBPE_API int  mbpe_splitter_create(int device_id, const char *pattern, mbpe_splitter **out);
MBPE_API void mbpe_splitter_destroy(mbpe_splitter *s);

/* Splits a text.
 *   text             n_bytes bytes of valid UTF-8; host memory, or -- text_on_device != 0 -- device memory of the
 *                    splitter's device, 16-byte aligned, read in place and never written.  (When a device text has
 *                    host spans, its bytes from the first of them to the last come back to the host in one copy.)
 *   endmask_dev_out  optional: 2 * ceil(n_bytes / 16) + 16 bytes of device memory, 16-byte aligned, which receive the
 *                    end mask mbpe_load_corpus_endmask takes: bit i & 7 of byte i >> 3 = text byte i is the last of
 *                    its chunk (the last byte of a non-empty text always is).  With NULL the mask stays in the
 *                    splitter (mbpe_splitter_endmask) until its next call
 *   chunk_off_out    optional, host, cap_chunks + 1 entries: the n_chunks + 1 offsets mbpe_presplit gives
 *   n_chunks_out     required.  The chunk count whenever the split succeeded: cap_chunks smaller than it (with
 *                    chunk_off_out given) returns MBPE_ERR_ARG and writes nothing else, so that a first call can
 *                    size the array.  Any other error leaves 0 there
 * MBPE_ERR_SPLIT_GAP, with neither mask nor offsets written: PCRE2 left bytes of a host span in no match, which only invalid UTF-8
 * brings about; mbpe_presplit handles such a text the reference's way. */
MBPE_API int  mbpe_splitter_split(mbpe_splitter *s, const uint8_t *text, uint64_t n_bytes, int text_on_device,
                                  uint8_t *endmask_dev_out, uint64_t *chunk_off_out, uint64_t cap_chunks,
                                  uint64_t *n_chunks_out);

/* Splits many texts in one call, around ranges that are not split: for every document on its own, what
 * Tokenizer::split_on_special followed by the regex split of every part does (Tokenizer.h:605-704), with the result
 * as an end mask over the original text instead of a rewritten buffer.
 *   text, n_bytes, text_on_device, endmask_dev_out   as for mbpe_splitter_split
 *   doc_off, n_docs  host, n_docs + 1 ascending offsets from 0 to n_bytes: document i is bytes [doc_off[i], doc_off[i + 1]).
 *                    A chunk never crosses a document boundary; an empty document has no chunk; n_docs == 0 or
 *                    n_bytes == 0 gives an empty result
 *   names, name_off, n_names   host: name j is names[name_off[j] .. name_off[j + 1]); n_names may be 0.  Every
 *                    occurrence of a non-empty name that lies inside one document is a candidate; candidates are
 *                    ordered by (position, name index) and one is TAKEN when it starts at or after the end of the
 *                    previous one taken in that document.  At most MBPE_SPLIT_MAX_NAMES names with
 *                    MBPE_SPLIT_MAX_NAME_BYTES bytes in all
 *   A PART is a maximal stretch of a document between taken occurrences.  A part whose first byte is NUL is not split
 *   (the reference's rule: such a part counts as special); every other part is split by the pattern as if it were a
 *   whole text -- so "a  " followed by "b" gives a, two spaces, b, where "a  b" gives a, one space, " b".
 *   ranges_out       optional, host, cap_ranges entries: ascending, the taken occurrences (name = index) and the
 *                    NUL-led parts (name = MBPE_SPLIT_RAW).  Each range is exactly one chunk of the mask
 *   n_ranges_out     optional: how many there are.  cap_ranges smaller than it (with ranges_out given) returns
 *                    MBPE_ERR_ARG after the count is stored and writes neither ranges nor endmask_dev_out.  With
 *                    ranges_out NULL they stay readable through mbpe_splitter_ranges
 *   n_chunks_out     required, as for mbpe_splitter_split
 * All arguments are checked before the device is touched.  MBPE_ERR_SPLIT_GAP as for mbpe_splitter_split: neither
 * mask nor ranges are written.  The mask stays readable through mbpe_splitter_endmask. */
#define MBPE_SPLIT_RAW            0xFFFFFFFFu
#define MBPE_SPLIT_MAX_NAMES      256u
#define MBPE_SPLIT_MAX_NAME_BYTES 16384u
typedef struct { uint64_t start, len; uint32_t name, pad; } mbpe_split_range;
MBPE_API int  mbpe_splitter_split_docs(mbpe_splitter *s, const uint8_t *text, uint64_t n_bytes, int text_on_device,
                                       const uint64_t *doc_off, uint64_t n_docs,
                                       const uint8_t *names, const uint64_t *name_off, uint32_t n_names,
                                       uint8_t *endmask_dev_out,
                                       mbpe_split_range *ranges_out, uint64_t cap_ranges, uint64_t *n_ranges_out,
                                       uint64_t *n_chunks_out);

/* The ranges of the latest successful mbpe_splitter_split_docs in the splitter's own host memory (valid until its
 * next call; none after mbpe_splitter_split), and the device time of that call's k_split_find launches (part of
 * mbpe_splitter_kernel_ms). */
MBPE_API int  mbpe_splitter_ranges(const mbpe_splitter *s, const mbpe_split_range **ranges_out, uint64_t *n_ranges_out);
MBPE_API int  mbpe_splitter_find_ms(const mbpe_splitter *s, float *ms_out);

/* The mask of the latest successful call in the splitter's own device memory (valid until its next call), its size,
 * and -- optional -- where that call's text is on the device: the caller's device text, or the splitter's copy of a
 * host text, so that a trainer can take it in place (mbpe_load_corpus_endmask with text_on_device) without a second
 * upload.  MBPE_ERR_STATE before the first successful call. */
MBPE_API int  mbpe_splitter_endmask(const mbpe_splitter *s, const uint8_t **endmask_dev_out, uint64_t *mask_bytes_out,
                                    const uint8_t **text_dev_out);

/*   "max_span"   the longest stretch between two sync points that the device walks (default MBPE_SPLIT_MAX_SPAN, at
 *                least 1); longer ones go to the host.  Same results.
 *   "unicode"    0 (default) or 1; any other value is MBPE_ERR_ARG.  1: stretches with bytes >= 0x80 are walked on the
 *                device too, as long as every UTF-8 sequence in them is well-formed (Unicode Table 3-7): the rule then
 *                reads scalar values, whose classes come from a table that PCRE2 itself fills once per process
 *                (mbpe_split_unicode_table; 278,528 bytes on the device), and a line break or -- gpt2 -- any whitespace
 *                but U+0020 in front of a non-whitespace character is a boundary as well.  A stretch with an
 *                ill-formed sequence, one cut inside a sequence, and one longer than "max_span" bytes stay host spans.
 *                Same results; mbpe_splitter_host_spans keeps its meaning.  MBPE_ERR_REGEX when PCRE2 cannot be asked.
 * The host spans are matched by up to MBPE_SPLIT_THREADS (environment; default 16) host threads, like mbpe_presplit. */
MBPE_API int  mbpe_splitter_set_option(mbpe_splitter *s, const char *name, int64_t value);

/* Device time of the latest call in milliseconds (HIP events on the splitter's stream around its kernels; copies
 * between host and device and the host's PCRE2 work are outside). */
MBPE_API int  mbpe_splitter_kernel_ms(const mbpe_splitter *s, float *ms_out);

/* Device allocations (hipMalloc calls) since the splitter was created.  A repeat call of no larger size leaves the
 * number as it is. */
MBPE_API int  mbpe_splitter_alloc_count(const mbpe_splitter *s, uint64_t *n_out);

/* The host spans of the latest call: how many, and (optional) the text bytes they hold. */
MBPE_API int  mbpe_splitter_host_spans(const mbpe_splitter *s, uint64_t *n_spans_out, uint64_t *n_bytes_out);

/* ---- chunk deduplication on the device (csrc/dedup.hip, dedup.h) ------------------------------------------------------
 * The distinct chunks of a chunked text in the order of their first occurrence, packed into one text with an end mask
 * in the layout mbpe_load_corpus_endmask reads, and for unique chunk j
 *   weights[j]      (u32) how often it occurs in the input; the weights add up to the input's chunk count
 *   first_chunk[j]  (u64) the index of its first occurrence among the input's chunks
 * Equality is decided by the bytes; the hash only places a chunk in a table, so the result is deterministic and
 * depends neither on the hash function nor on a collision.  Together with mbpe_load_corpus_endmask_weighted a training
 * runs on the unique chunks and still counts what the whole corpus holds.
 *
 * A deduper has its own non-blocking stream and owns its device buffers; a repeat call of no larger size allocates
 * nothing (mbpe_dedup_alloc_count).  Device memory: 16 B per chunk (end offset, table position) plus a table of
 * 12 B x the power of two at or above 2 x n_chunks (24 .. 48 B per chunk), 16 B per 256 chunks and 8 B per 16 KiB of
 * text for the scans; the result takes 1 1/8 B per unique byte and 12 B per unique chunk.  mbpe_dedup_chunks adds the
 * uploaded text (host text only), 1/8 B per byte for its mask and, with empty chunks, 8 B per chunk.
 *
 *   mbpe_dedup_chunks_endmask  text_dev (16-byte aligned) and endmask_dev (4-byte aligned, the layout of
 *                              mbpe_splitter_split) are read in place.  Bytes behind the last end bit belong to no
 *                              chunk.  2^32 - 1 chunks or more: MBPE_ERR_ARG, here once the device has counted them.
 *   mbpe_dedup_chunks          chunk_off as for mbpe_load_corpus (host, required); the mask is built on the host the same
 *                              way, except that the NUL rule is not applied: deduplication is about bytes.  Empty
 *                              chunks vanish; first_chunk still counts them.  n_chunks >= 2^32 - 1 is MBPE_ERR_ARG.
 *   n_unique_out (required), n_unique_bytes_out (optional)   the result's sizes
 *   mbpe_dedup_result          device views of the latest result, valid until the deduper's next call (any may be NULL)
 *   mbpe_dedup_get             host copies: text_out (cap_bytes), chunk_off_out (cap_chunks + 1 offsets), weights_out and
 *                              first_chunk_out (cap_chunks each); any may be NULL.  A cap below the size the dedup
 *                              call reported is MBPE_ERR_ARG and nothing is written.
 *   options   "max_chunk_bytes"  default 256: a longer chunk is never hashed and passes through as a unique chunk of
 *                                weight 1 at its place (a duplicate of it appears twice: still exact)
 *             "hash_bits"        default 64; 0 .. 64: the hash is cut to that many bits (tests: collisions)
 * Arguments are checked before the device is touched.  No CPU fallback: MBPE_ERR_NO_DEVICE without a HIP device. */
typedef struct mbpe_dedup mbpe_dedup;
MBPE_API int  mbpe_dedup_create(int device_id, mbpe_dedup **out);
MBPE_API void mbpe_dedup_destroy(mbpe_dedup *d);
MBPE_API int  mbpe_dedup_chunks_endmask(mbpe_dedup *d, const uint8_t *text_dev, uint64_t n_bytes, const uint8_t *endmask_dev,
                                        uint64_t *n_unique_out, uint64_t *n_unique_bytes_out);
MBPE_API int  mbpe_dedup_chunks(mbpe_dedup *d, const uint8_t *text, uint64_t n_bytes, int text_on_device,
                                const uint64_t *chunk_off, uint64_t n_chunks, uint64_t *n_unique_out,
                                uint64_t *n_unique_bytes_out);
MBPE_API int  mbpe_dedup_result(const mbpe_dedup *d, const uint8_t **text_dev_out, const uint8_t **endmask_dev_out,
                                const uint32_t **weights_dev_out, const uint64_t **first_chunk_dev_out);
MBPE_API int  mbpe_dedup_get(mbpe_dedup *d, uint8_t *text_out, uint64_t *chunk_off_out, uint32_t *weights_out,
                             uint64_t *first_chunk_out, uint64_t cap_bytes, uint64_t cap_chunks);
MBPE_API int  mbpe_dedup_set_option(mbpe_dedup *d, const char *name, int64_t value);
MBPE_API int  mbpe_dedup_kernel_ms(const mbpe_dedup *d, float *ms_out);
MBPE_API int  mbpe_dedup_alloc_count(const mbpe_dedup *d, uint64_t *n_out);

/* The inverse map: unique_of[c] (u32) = the index j of the unique chunk that has chunk c's bytes, for every chunk the
 * deduper kept (the empty chunks of mbpe_dedup_chunks stay out, as everywhere; a chunk that passed through unhashed is
 * its own unique chunk).  Computed only while the option "map" is 1 (default 0: the deduper launches and allocates
 * exactly what it does without it); it costs one more short kernel and 4 B per chunk.  Any other value is MBPE_ERR_ARG.
 *   mbpe_dedup_map      device view of the latest result and the number of chunks it speaks of, valid until the
 *                       deduper's next call (either may be NULL)
 *   mbpe_dedup_get_map  host copy; unique_of_out NULL: n_chunks_out receives the count only.  A cap below it is
 *                       MBPE_ERR_ARG and nothing is written
 * MBPE_ERR_STATE when the latest dedup did not succeed or ran without the option. */
MBPE_API int  mbpe_dedup_map(const mbpe_dedup *d, const uint32_t **unique_of_dev_out, uint64_t *n_chunks_out);
MBPE_API int  mbpe_dedup_get_map(mbpe_dedup *d, uint32_t *unique_of_out, uint64_t cap_chunks, uint64_t *n_chunks_out);

/* ---- word counts across calls (csrc/wordcount.hip, wordcount.h) --------------------------------------------------------
 * A corpus that arrives in pieces: every add call dedups its piece on the device (an owned mbpe_dedup) and folds the
 * result into a table the object keeps there.  With piece p's chunk list L_p (empty chunks dropped), the table after
 * L_0, L_1, ... holds the unique chunks, weights and first occurrences of ONE dedup of the concatenated list
 * L_0 + L_1 + ...: first-occurrence order over the concatenation, first_chunk the index in it, and a chunk above
 * "max_chunk_bytes" once per occurrence with weight 1.  Training on it (mbpe_load_corpus_*_weighted) therefore equals
 * training on the concatenated list, for both tie-breaks.  Pieces are split independently: a piece boundary is a chunk
 * boundary.  Device memory while counting: the deduper's for the largest piece (see mbpe_dedup_*) plus, per unique
 * chunk, its bytes, 24 B and 16 .. 32 B of table; host memory: one piece.
 *
 *   mbpe_wordcount_add_endmask  a piece as device text with an end mask; mbpe_wordcount_add: as text with chunk_off.
 *                               Argument conventions, layouts and alignment are those of mbpe_dedup_chunks_endmask and
 *                               mbpe_dedup_chunks (first_chunk counts the empty chunks of chunk_off).  repeat >= 1 counts
 *                               the piece that many times, written out back to back: the weights are multiplied, order
 *                               and first_chunk are those of one copy, and the chunks after it move on by repeat x the
 *                               piece's; 0 is MBPE_ERR_ARG.  n_unique_total_out (required) and
 *                               n_unique_bytes_total_out (optional): the table's sizes after the call.  2^32 - 1 unique
 *                               chunks or more: MBPE_ERR_ARG.  A later call that brings no new chunk and is no larger
 *                               than an earlier piece allocates nothing (mbpe_wordcount_alloc_count).
 *   mbpe_wordcount_result       device views: the packed text, its end mask in the layout mbpe_load_corpus_endmask reads,
 *                               the weights as u32 and first_chunk (u64); any may be NULL.  Valid until the next add or
 *                               reset; they go into mbpe_load_corpus_endmask_weighted(..., weights_on_device = 1) as they
 *                               are.
 *   mbpe_wordcount_get          host copies, as mbpe_dedup_get
 *   A weight that reaches 2^31 (the limit of the weighted load; the u64 sums saturate) makes _result and _get return
 *   MBPE_ERR_OVERFLOW until mbpe_wordcount_reset.
 *   mbpe_wordcount_stats        pieces added, chunks counted (repeats included), unique chunks and their bytes
 *   mbpe_wordcount_reset        empty again, buffers kept
 *   mbpe_wordcount_set_option   "max_chunk_bytes", "hash_bits": handed to the owned deduper, same defaults and ranges;
 *                               MBPE_ERR_STATE once a piece has been added (until the next reset)
 *   mbpe_wordcount_kernel_ms    device time of the latest add or merge call: the deduper's kernels (add) and the fold's,
 *                               for mbpe_wordcount_merge_blob with the check of the incoming chunks
 * Arguments are checked before the device is touched.  No CPU fallback: MBPE_ERR_NO_DEVICE without a HIP device.
 *
 * Tables merge, so the counting can be spread over devices, processes and days, and be checkpointed.  Let A be the count
 * of pieces P_0 .. P_{i-1} and B, a fresh object with the same "max_chunk_bytes", the count of P_i .. P_{k-1}.  After
 * merging B into A, A is, bit for bit, the table of counting P_0 .. P_{k-1} into one object: text, ends, u64 weights,
 * first_chunk, the chunks above "max_chunk_bytes" once per occurrence, and the totals.  Per entry of B: found in A -> its
 * weight is added; not found -> appended in B's order with first_chunk = A's chunks so far + B's first_chunk; above
 * "max_chunk_bytes" -> appended without a look; then A's chunks so far, chunks counted and pieces grow by B's.  Merging
 * in piece order is therefore associative: a chain ((A + B) + C) and a tree (A + (B + C)) give the same table, and a
 * training on it is the training on all pieces.  Merging out of order is allowed and gives the table of the pieces in
 * that order: the weights are the same, the order of the entries and first_chunk -- what the `first` tie-break sees --
 * are those of that order.  A weight that reaches 2^31 sets the sticky overflow as an add does.  Moving a blob between
 * processes or machines is the caller's business (files, torch.distributed.all_gather_object, MPI).
 *   mbpe_wordcount_export_size, mbpe_wordcount_export
 *       the table as a host blob; the object is unchanged and goes on counting, so an export is also a checkpoint.
 *       Little-endian: a 64-byte header (u32 magic "MBWC", u32 version 1, then u64 max_chunk_bytes, n_unique, n_bytes,
 *       n_pieces, n_chunks_total, chunk_base -- the chunks of the concatenated list, empty ones included -- and a u64
 *       that is 0), then ends, weights and first_chunk (n_unique u64 each), then the text padded with zeros to 16
 *       bytes.  "hash_bits" is not in it: it places slots and decides nothing.  A cap below the size is MBPE_ERR_ARG;
 *       an overflowed table MBPE_ERR_OVERFLOW, as for mbpe_wordcount_get.  n_bytes_out of _export may be NULL.
 *   mbpe_wordcount_merge_blob
 *       checks, uploads and folds a blob; into an empty object it is an import (exporting again gives the same
 *       bytes).  The outputs (either may be NULL) are the table's sizes after the call.  A blob is not trusted: it is
 *       refused with MBPE_ERR_ARG and a message naming the rule when the magic or the version is wrong; when the sizes do
 *       not give the blob's length; when the ends are not strictly ascending or do not end at n_bytes; when a weight
 *       is 0; when first_chunk is not strictly ascending or not below chunk_base; when the weights' sum is not
 *       n_chunks_total; when it was counted with another "max_chunk_bytes"; and when two of its chunks at or below
 *       "max_chunk_bytes" have the same bytes (checked on the device in a scratch table).  All of this comes before any
 *       weight of the object is touched: a refused merge leaves the table, its statistics and its views as they were.
 *   mbpe_wordcount_merge
 *       the same fold straight from the device buffers of `other`, which stays unchanged; no check is needed.
 *       MBPE_ERR_ARG when the objects are on different devices (use the blob there), when w == other, and when their
 *       options differ; MBPE_ERR_OVERFLOW when `other` has overflowed.
 *   A merge that fails later, in an allocation or on the device, leaves the object as a failed add does: weights of
 *   entries that were found may have grown; reset it. */
typedef struct mbpe_wordcount mbpe_wordcount;
MBPE_API int  mbpe_wordcount_create(int device_id, mbpe_wordcount **out);
MBPE_API void mbpe_wordcount_destroy(mbpe_wordcount *w);
MBPE_API int  mbpe_wordcount_add_endmask(mbpe_wordcount *w, const uint8_t *text_dev, uint64_t n_bytes,
                                         const uint8_t *endmask_dev, uint32_t repeat, uint64_t *n_unique_total_out,
                                         uint64_t *n_unique_bytes_total_out);
MBPE_API int  mbpe_wordcount_add(mbpe_wordcount *w, const uint8_t *text, uint64_t n_bytes, int text_on_device,
                                 const uint64_t *chunk_off, uint64_t n_chunks, uint32_t repeat,
                                 uint64_t *n_unique_total_out, uint64_t *n_unique_bytes_total_out);
MBPE_API int  mbpe_wordcount_result(mbpe_wordcount *w, const uint8_t **text_dev_out, const uint8_t **endmask_dev_out,
                                    const uint32_t **weights_dev_out, const uint64_t **first_chunk_dev_out);
MBPE_API int  mbpe_wordcount_get(mbpe_wordcount *w, uint8_t *text_out, uint64_t *chunk_off_out, uint32_t *weights_out,
                                 uint64_t *first_chunk_out, uint64_t cap_bytes, uint64_t cap_chunks);
MBPE_API int  mbpe_wordcount_stats(const mbpe_wordcount *w, uint64_t *n_pieces_out, uint64_t *n_chunks_total_out,
                                   uint64_t *n_unique_out, uint64_t *n_unique_bytes_out);
MBPE_API int  mbpe_wordcount_reset(mbpe_wordcount *w);
MBPE_API int  mbpe_wordcount_set_option(mbpe_wordcount *w, const char *name, int64_t value);
MBPE_API int  mbpe_wordcount_kernel_ms(const mbpe_wordcount *w, float *ms_out);
MBPE_API int  mbpe_wordcount_alloc_count(const mbpe_wordcount *w, uint64_t *n_out);
MBPE_API int  mbpe_wordcount_export_size(const mbpe_wordcount *w, uint64_t *n_bytes_out);
MBPE_API int  mbpe_wordcount_export(mbpe_wordcount *w, uint8_t *blob_out, uint64_t cap_bytes, uint64_t *n_bytes_out);
MBPE_API int  mbpe_wordcount_merge_blob(mbpe_wordcount *w, const uint8_t *blob, uint64_t n_bytes,
                                        uint64_t *n_unique_total_out, uint64_t *n_unique_bytes_total_out);
MBPE_API int  mbpe_wordcount_merge(mbpe_wordcount *w, const mbpe_wordcount *other);

/* ---- token frequency tables (csrc/hist.hip, hist.h) -----------------------------------------------------------------
 * How often every token id is used, counted on the device in 64 bits, exact: no floating point and no 32-bit
 * intermediate that can wrap (a workgroup's private 32-bit counters are flushed before 2^32 adds; hist.h).  With T the
 * tokens the corresponding encode call would return for the same arguments and encoder state (order, dropout and
 * seed, "dedup", pieces, NUL-led chunks, singles):
 *     counts[id] += repeat * |{ j : T[j] == id }|   for id < n_ids
 *     n_other    += repeat * |{ j : T[j] >= n_ids }|
 *     n_tokens   += repeat * |T|
 * so sum(counts) + n_other == n_tokens always.  A call that returns an error leaves the table exactly as it was.
 *
 * mbpe_token_counts: tokens that exist already.  The conventions of mbpe_pack_tokens: token_bits 32 (bit 31 is cleared
 * on read) or 16 (plain ids, 65,535 is one), host or device (tokens_on_device; a device pointer aligned to its
 * elements).  WRITES counts_out[0 .. n_ids) (host, or device with out_on_device: 8-byte aligned) and *n_other_out
 * (required, host).  n_ids must lie in 1 .. MBPE_MAX_COUNT_IDS; that, an unknown token_bits, more than 2^40 tokens
 * and a misaligned device pointer are MBPE_ERR_ARG before the device is touched.  n_tokens == 0 gives zeros.
 * mbpe_token_counts_kernel_ms: the device time of the calling thread's latest such call (the histogram kernel alone).
 *
 * mbpe_encoder_count, mbpe_encoder_count_endmask: mbpe_encoder_encode and mbpe_encoder_encode_endmask called as a
 * query (tokens_out NULL), plus the count; no token leaves the device.  Argument checks, error codes, pieces (the
 * passes run once), the NUL rule, singles, "rank_order" and dropout hold as they do there.  With "dedup" 1 they take
 * that route WITHOUT the expansion: the count of the whole text is the count of the table of token runs, every run
 * weighted by how many chunks copy it, and those weights are the histogram of the patched unique_of map (which
 * handles one-token chunks and the empty run by construction).  Dropout > 0 with "dedup" stays MBPE_ERR_ARG.
 *   repeat            at least 1 (0: MBPE_ERR_ARG): the text counts that many times, as for mbpe_wordcount_add
 *   n_tokens_out      required: |T|, without repeat
 * Overflow is decided on the host before the device is touched: with S the weighted token total the table has
 * reached, S + n_bytes * repeat >= 2^64 is MBPE_ERR_OVERFLOW.  Encoding never makes more tokens than bytes and every
 * bin is at most the total, so no bin can wrap.
 * The table has n_ids = max(256 + n_merges, option "count_ids") entries; ids at or beyond it (one-token chunks only)
 * are counted in n_other.  "count_ids" is 0 (the default) .. MBPE_MAX_COUNT_IDS (else MBPE_ERR_ARG) and MBPE_ERR_STATE
 * once something has been counted and not reset; 256 + n_merges above MBPE_MAX_COUNT_IDS is MBPE_ERR_VOCAB from the
 * first count call.  Every call counts into a scratch table of the call's own and folds it into the kept one
 * (kept[i] += repeat * call[i]) after everything that can fail has succeeded.  The table and its scratch (16 bytes
 * per id; on the "dedup" route 8 bytes per table run in addition) are allocated by the first count call: an encoder
 * that is never asked to count launches and allocates exactly what it did before, and mbpe_encoder_alloc_count of
 * the other calls is unchanged.  A repeat count call of no larger size allocates nothing.  mbpe_encoder_kernel_ms
 * includes the histogram and the fold.
 *   mbpe_encoder_counts        copies the table: counts_out (cap_ids entries, host or device; fewer than n_ids is
 *                              MBPE_ERR_ARG; NULL: query), and n_ids, n_other and the weighted token total (each
 *                              pointer may be NULL)
 *   mbpe_encoder_counts_reset  zeroes the table and the totals; "count_ids" may change again */
#define MBPE_MAX_COUNT_IDS 33554432u   /* 2^25 */
MBPE_API int  mbpe_token_counts(int device_id, const void *tokens, uint64_t n_tokens, uint32_t token_bits,
                                int tokens_on_device, uint64_t *counts_out, uint64_t n_ids, int out_on_device,
                                uint64_t *n_other_out);
MBPE_API int  mbpe_token_counts_kernel_ms(float *ms_out);
MBPE_API int  mbpe_encoder_count(mbpe_encoder *e, const uint8_t *text, uint64_t n_bytes, int text_on_device,
                                 const uint64_t *chunk_off, uint64_t n_chunks, uint64_t repeat, uint64_t *n_tokens_out,
                                 uint32_t *n_passes_out);
MBPE_API int  mbpe_encoder_count_endmask(mbpe_encoder *e, const uint8_t *text_dev, uint64_t n_bytes,
                                         const uint8_t *endmask_dev, const mbpe_single *singles, uint64_t n_singles,
                                         uint64_t repeat, uint64_t *n_tokens_out, uint32_t *n_passes_out);
MBPE_API int  mbpe_encoder_counts(mbpe_encoder *e, uint64_t *counts_out, uint64_t cap_ids, int out_on_device,
                                  uint64_t *n_ids_out, uint64_t *n_other_out, uint64_t *n_tokens_out);
MBPE_API int  mbpe_encoder_counts_reset(mbpe_encoder *e);

#ifdef __cplusplus
}
#endif
#endif /* MBPE_H */
