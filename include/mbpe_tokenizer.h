/*
 * mbpe_tokenizer.h -- C-ABI of the host-side mirror of minbpe-cc's Tokenizer
 * (code/include/Tokenizer.h:379-927): the pieces around the GPU hot path that a
 * drop-in needs -- regex pre-split, "minbpe v1" model files, special tokens,
 * encode, decode -- plus train(), which runs the hot path through mbpe.h.
 * The C++ class behind it is minbpe-cc_amd/host/tokenizer.h (same method names
 * and argument meaning as the reference class); the `minbpe-cc` executable
 * built from host/main.cpp keeps the reference's command line.
 *
 * Return codes are mbpe_status values (mbpe.h); text of the last error:
 * mbpe_last_error().
 */
#ifndef MBPE_TOKENIZER_H
#define MBPE_TOKENIZER_H

#include "mbpe.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mbpe_tokenizer mbpe_tokenizer;

/* Tokenizer(const string &pattern), Tokenizer.h:391-451 ("" = basic). */
MBPE_API int  mbpe_tok_create(const char *pattern, mbpe_tokenizer **out);
MBPE_API void mbpe_tok_destroy(mbpe_tokenizer *t);

/* set_special_tokens_from_file, Tokenizer.h:476-486: "name id" pairs. */
MBPE_API int mbpe_tok_set_special_tokens(mbpe_tokenizer *t, const char *text, uint64_t n);

/* train, Tokenizer.h:489-598.  conflict_resolution: 1 = lexical, 0 = first
 * (the reference CLI's default); both run on HIP device `device_id` through
 * mbpe_train. */
MBPE_API int mbpe_tok_train(mbpe_tokenizer *t, const uint8_t *text, uint64_t n, uint32_t vocab_size,
                            int conflict_resolution, int verbose, int device_id);

/* The same with the gpt2 / gpt4 pre-split on the device as well (mbpe_splitter_split, then
 * mbpe_load_corpus_endmask on the text the splitter uploaded): same merges.  A tokenizer whose pattern is not one of
 * the two built-in ones returns MBPE_ERR_ARG; it does not fall back to the host split. */
MBPE_API int mbpe_tok_train_split_device(mbpe_tokenizer *t, const uint8_t *text, uint64_t n, uint32_t vocab_size,
                                         int conflict_resolution, int verbose, int device_id);

/* Continues a training: the tokenizer's current merges -- loaded, set or trained -- are the prior table of
 * mbpe_train_begin_from (mbpe.h), the training adds merges up to vocab_size on `text`, and on success the tokenizer
 * holds prior + new merges, which mbpe_tok_save writes.  Pattern and special tokens stay.  device_split != 0 takes the
 * route of mbpe_tok_train_split_device (and honours mbpe_tok_set_split_unicode).  Verbose prints the per-merge line
 * of the new merges only.  A tokenizer without merges behaves like mbpe_tok_train.  Errors keep the code of the call
 * that failed: MBPE_ERR_ARG for a vocab_size below the tokens the model has or a table mbpe_merges_check refuses (the
 * tokenizer is unchanged then), MBPE_ERR_VOCAB beyond MBPE_MAX_VOCAB_WIDE (beyond the 16-bit slot format the training
 * continues on 32-bit tokens: the context option "resume_wide" is set), MBPE_ERR_OOM above the encoder's one-piece
 * limit. */
MBPE_API int mbpe_tok_train_continue(mbpe_tokenizer *t, const uint8_t *text, uint64_t n, uint32_t vocab_size,
                                     int conflict_resolution, int verbose, int device_id, int device_split);

/* Training on a corpus that arrives in pieces -- many files, more than one host buffer or more than device memory holds.
 * The pieces' chunks are counted on the device as they pass (mbpe_wordcount_*, mbpe.h) and the training runs on the
 * table: the merges, counts, verbose lines, .model and .vocab of a training on the pieces' chunk lists laid end to end,
 * for both tie-breaks.  Every piece is split on its own, so a piece boundary is a chunk boundary ("a  " + "b" is not
 * "a  b"); cut where a letter or digit is followed by whitespace -- a chunk boundary under gpt2 and gpt4 -- and the
 * pieces give the whole text's result.  Host memory: one piece; device memory while counting: the largest piece's
 * split and dedup plus the unique chunks.  The training is that of mbpe_tok_set_train_dedup: one rank (the counting
 * can be spread over devices, processes and runs: _export and _merge below), the 32-bit loop, and a chunk above 256
 * bytes is never merged with its duplicates.
 *   _begin   opens the session on device_id; device_split != 0: the pieces are split on the device too.
 *            MBPE_ERR_STATE while a session is open.
 *   _add     one piece, counted `repeat` (>= 1, else MBPE_ERR_ARG) times, as if written out back to back: how a data mix
 *            up-weights a source.  With the device split (one splitter for the session, mbpe_tok_set_split_unicode
 *            honoured by every add) neither text nor mask returns to the host; a pattern that is not gpt2 / gpt4 is
 *            MBPE_ERR_ARG there, as for mbpe_tok_train_split_device.  MBPE_ERR_STATE without a session.  A failed add
 *            leaves the session open; the tokenizer's merges are untouched.
 *   _finish  loads the table into a fresh context -- in place after the device split; after the host split the unique
 *            chunks come back once and go through mbpe_load_corpus_weighted, so the NUL rule is applied as ever -- and
 *            trains as mbpe_tok_train does.  resume != 0 continues from the merges the tokenizer holds, with the checks
 *            and error codes of mbpe_tok_train_continue.  Verbose prints "Split input text into N chunks" once, with
 *            the session's total, and the length in the closing line is the whole corpus's.  The tokenizer's merges
 *            change only when it succeeds; the session is closed either way.
 *   _abort   closes the session, if any.  After _finish or _abort the session's device objects are gone.
 * The counting can be spread over devices, processes and runs; the training stage stays one rank.
 *   _export_size, _export   the open session's counts as a host blob: 32 bytes (u32 magic "MBTC", u32 version 1, u64
 *            length of the split pattern, u64 chunks and u64 bytes the session has seen), the pattern padded with zeros
 *            to 8 bytes, then the blob of mbpe_wordcount_export (mbpe.h).  The session stays open and goes on counting:
 *            an export is also a checkpoint.  A cap below the size is MBPE_ERR_ARG; n_bytes_out of _export may be NULL.
 *   _merge   merges a blob into the open session as mbpe_wordcount_merge_blob does -- the session becomes the count of
 *            its own pieces followed by the blob's, with the checks listed there -- and adds the blob's chunks and bytes
 *            to the totals that the verbose lines of _finish report, so a session that merged the blobs of all pieces
 *            trains and prints like one that was given all pieces.  Host split and either device split give the same
 *            chunks: sessions counted on different routes merge freely.  A blob counted under another split pattern,
 *            or one that is truncated or not a counts blob, is MBPE_ERR_ARG; the session is unchanged then.  Merged out
 *            of piece order, the `first` tie-break sees the first occurrences of that order.
 *   All three return MBPE_ERR_STATE without a session.  How a blob travels is the caller's business. */
MBPE_API int mbpe_tok_train_pieces_begin(mbpe_tokenizer *t, int device_id, int device_split);
MBPE_API int mbpe_tok_train_pieces_add(mbpe_tokenizer *t, const uint8_t *text, uint64_t n, uint32_t repeat);
MBPE_API int mbpe_tok_train_pieces_finish(mbpe_tokenizer *t, uint32_t vocab_size, int conflict_resolution, int verbose,
                                          int resume);
MBPE_API int mbpe_tok_train_pieces_abort(mbpe_tokenizer *t);
MBPE_API int mbpe_tok_train_pieces_export_size(mbpe_tokenizer *t, uint64_t *n_bytes_out);
MBPE_API int mbpe_tok_train_pieces_export(mbpe_tokenizer *t, uint8_t *blob_out, uint64_t cap_bytes, uint64_t *n_bytes_out);
MBPE_API int mbpe_tok_train_pieces_merge(mbpe_tokenizer *t, const uint8_t *blob, uint64_t n_bytes);

/* Direct access to the trained / loaded merges (2 u32 per merge). */
MBPE_API int mbpe_tok_set_merges(mbpe_tokenizer *t, const uint32_t *merges, uint32_t n_merges);
MBPE_API int mbpe_tok_get_merges(mbpe_tokenizer *t, uint32_t *merges_out, uint32_t cap, uint32_t *n_out);

/* save / load, Tokenizer.h:875-926 / :754-872. */
MBPE_API int mbpe_tok_save(mbpe_tokenizer *t, const char *path, int write_vocab);
MBPE_API int mbpe_tok_load(mbpe_tokenizer *t, const char *path, int verbose);

/* encode, Tokenizer.h:653-722 (special split :605-650, regex split :664-704,
 * greedy multi-pass merge application :325-367).  tokens_out may be NULL to
 * query the count. */
MBPE_API int mbpe_tok_encode(mbpe_tokenizer *t, const uint8_t *text, uint64_t n, int verbose,
                             uint32_t *tokens_out, uint64_t cap, uint64_t *n_out);

/* The same with internal_encode (Tokenizer.h:325-377) on HIP device `device_id`
 * (mbpe_encoder_encode, with an encoder that the tokenizer keeps until its merges change
 * or another device is named); special-token and regex splitting stay on the host.  No CPU
 * fallback: MBPE_ERR_NO_DEVICE without a device. */
MBPE_API int mbpe_tok_encode_device(mbpe_tokenizer *t, const uint8_t *text, uint64_t n, int verbose, int device_id,
                                    uint32_t *tokens_out, uint64_t cap, uint64_t *n_out);

/* encode of n_docs documents in one device call.  Document i is text[doc_off[i] .. doc_off[i + 1]) (n_docs + 1
 * ascending offsets, host memory); every document is split on special tokens and by the pattern on its own, so no
 * chunk spans two documents, and all chunks go to the device in ONE mbpe_encoder_encode.  tokens_out (NULL: query)
 * receives the documents' tokens one after the other, doc_tok_off_out (optional, n_docs + 1; also on a query) where each begins:
 * document i is tokens_out[doc_tok_off_out[i] .. doc_tok_off_out[i + 1]) and equals mbpe_tok_encode of that
 * document; an empty document has no tokens.  n_out is required; device_id must not be negative. */
MBPE_API int mbpe_tok_encode_batch_device(mbpe_tokenizer *t, const uint8_t *text, const uint64_t *doc_off,
                                          uint64_t n_docs, int verbose, int device_id, uint32_t *tokens_out,
                                          uint64_t cap, uint64_t *doc_tok_off_out, uint64_t *n_out);

/* encode with token byte ranges ("offsets mapping"): the tokens of mbpe_tok_encode / mbpe_tok_encode_device and, for
 * token j, ranges_out[2j] and ranges_out[2j + 1]: the start and the end of the bytes it stands for in the ORIGINAL text,
 * relative to its document's first byte.  They are pairs and not a tiling because the encoder does not always read the
 * original text: with the host split a special token is replaced by a "\0<id>" marker and a custom pattern may leave
 * bytes between two matches that belong to no token.  The ranges ascend and do not overlap; text[start .. end) is the
 * token's vocabulary entry, or -- a special token -- the occurrence of its name.
 *   device_id < 0    (single-text call only) the host loop: text_to_vector, the merge loop in the order
 *                    mbpe_tok_set_encode_order chose, ranges from the vocabulary's entry lengths within each chunk
 *   device_id >= 0   mbpe_encoder_encode_byteoff over the host split, whose chunks carry their source ranges (a chunk's
 *                    first token starts where its source starts, its last one ends where it ends), or -- after
 *                    mbpe_tok_set_encode_split(1) -- mbpe_encoder_encode_endmask_byteoff over the device split, whose
 *                    text is the original text.  mbpe_tok_set_split_unicode holds as for the plain calls.  The device
 *                    routes need merges mbpe_merges_check accepts (MBPE_ERR_ARG otherwise)
 * The three routes agree token for token and range for range.  tokens_out NULL: query (n_out, and doc_tok_off_out
 * where given); otherwise ranges_out (2 * cap entries) is required.  A cap too small returns MBPE_ERR_ARG, writes no
 * token and no range and still reports the count.  The batch call is mbpe_tok_encode_batch_device with ranges_out
 * added: one device call for all documents, each equal to the single-text call on it. */
MBPE_API int mbpe_tok_encode_byteoff(mbpe_tokenizer *t, const uint8_t *text, uint64_t n, int verbose, int device_id,
                                     uint32_t *tokens_out, uint64_t *ranges_out, uint64_t cap, uint64_t *n_out);
MBPE_API int mbpe_tok_encode_batch_byteoff_device(mbpe_tokenizer *t, const uint8_t *text, const uint64_t *doc_off,
                                                  uint64_t n_docs, int verbose, int device_id, uint32_t *tokens_out,
                                                  uint64_t *ranges_out, uint64_t cap, uint64_t *doc_tok_off_out,
                                                  uint64_t *n_out);

/* The same documents as one id matrix on the device: every document is split as above, all chunks go to the device
 * in ONE mbpe_encoder_encode_batch (mbpe.h), which encodes them and packs the documents by `spec`.  bos_id and eos_id
 * may name special-token ids.  spec, ids_out (NULL: query), cap_rows, out_on_device, len_out, n_rows_out (required)
 * and n_tokens_out (optional) are those of mbpe_encoder_encode_batch.  A PADDED row i is document i: its first (or
 * last) tokens of mbpe_tok_encode. */
MBPE_API int mbpe_tok_encode_batch_packed_device(mbpe_tokenizer *t, const uint8_t *text, const uint64_t *doc_off,
                                                 uint64_t n_docs, int verbose, int device_id,
                                                 const mbpe_pack_spec *spec, void *ids_out, uint64_t cap_rows,
                                                 int out_on_device, uint32_t *len_out, uint64_t *n_rows_out,
                                                 uint64_t *n_tokens_out);

/* The same with the training-batch outputs of mbpe_encoder_encode_batch_aux (mbpe.h): labels, positions and segments
 * per `aux` (required), and the documents' token offsets in doc_tok_off_out (optional, host, n_docs + 1), which
 * mbpe_pack_cu_seqlens takes. */
MBPE_API int mbpe_tok_encode_batch_aux_device(mbpe_tokenizer *t, const uint8_t *text, const uint64_t *doc_off,
                                              uint64_t n_docs, int verbose, int device_id, const mbpe_pack_spec *spec,
                                              void *ids_out, uint64_t cap_rows, int out_on_device, uint32_t *len_out,
                                              uint64_t *n_rows_out, uint64_t *n_tokens_out, const mbpe_pack_aux *aux,
                                              uint64_t *doc_tok_off_out);

/* The same documents as an encoder-decoder batch by span corruption (mbpe.h, which holds the rule): the arguments of
 * mbpe_tok_encode_batch_aux_device up to device_id, then dn, the two specs and the output struct of
 * mbpe_encoder_encode_batch_denoise in place of spec / aux.  One row per unit: with dn->segment_tokens a long text
 * becomes several rows, out->row_doc says whose.  The call goes to mbpe_encoder_encode_batch_denoise or --
 * mbpe_tok_set_encode_split -- mbpe_encoder_encode_batch_endmask_denoise, and mbpe_tok_set_encode_order, _dropout,
 * _dedup and _split_unicode hold as for the other batch calls.  The sentinels may be special-token ids: the stage
 * writes ids and never looks them up.  While mbpe_tok_set_encode_fim or _mlm is on the call is MBPE_ERR_ARG. */
MBPE_API int mbpe_tok_encode_batch_denoise_device(mbpe_tokenizer *t, const uint8_t *text, const uint64_t *doc_off,
                                                  uint64_t n_docs, int verbose, int device_id,
                                                  const mbpe_denoise_spec *dn, const mbpe_pack_spec *enc_spec,
                                                  const mbpe_pack_spec *dec_spec, const mbpe_denoise_batch *out,
                                                  uint64_t cap_rows, int out_on_device, uint64_t *n_rows_out,
                                                  uint64_t *n_tokens_out);

/* The same for the window layout of mbpe_pack_windows (mbpe.h): a text that does not fit a row becomes several rows
 * that share win->stride tokens.  The arguments of mbpe_tok_encode_batch_aux_device, then win (required); the call goes
 * to mbpe_encoder_encode_batch_windows or -- mbpe_tok_set_encode_split -- mbpe_encoder_encode_batch_endmask_windows, and
 * mbpe_tok_set_encode_order, _dropout, _dedup and _split_unicode hold as for the other batch calls. */
MBPE_API int mbpe_tok_encode_batch_windows_device(mbpe_tokenizer *t, const uint8_t *text, const uint64_t *doc_off,
                                                  uint64_t n_docs, int verbose, int device_id,
                                                  const mbpe_pack_spec *spec, void *ids_out, uint64_t cap_rows,
                                                  int out_on_device, uint32_t *len_out, uint64_t *n_rows_out,
                                                  uint64_t *n_tokens_out, const mbpe_pack_aux *aux,
                                                  uint64_t *doc_tok_off_out, const mbpe_pack_window *win);

/* The same for the fit layout of mbpe_pack_fit (mbpe.h): whole texts, many per row, placed by best fit; a text is cut
 * only where it is longer than a row.  The arguments of mbpe_tok_encode_batch_aux_device, then fit (required; spec->layout
 * MBPE_PACK_PACKED); the call goes to mbpe_encoder_encode_batch_fit or -- mbpe_tok_set_encode_split --
 * mbpe_encoder_encode_batch_endmask_fit, and mbpe_tok_set_encode_order, _dropout, _dedup and _split_unicode hold as for
 * the other batch calls. */
MBPE_API int mbpe_tok_encode_batch_fit_device(mbpe_tokenizer *t, const uint8_t *text, const uint64_t *doc_off,
                                              uint64_t n_docs, int verbose, int device_id, const mbpe_pack_spec *spec,
                                              void *ids_out, uint64_t cap_rows, int out_on_device, uint32_t *len_out,
                                              uint64_t *n_rows_out, uint64_t *n_tokens_out, const mbpe_pack_aux *aux,
                                              uint64_t *doc_tok_off_out, const struct mbpe_pack_fit *fit);

/* Where the mbpe_tok_encode*_device calls above split their text: 0 (the default) on the host, as described there;
 * otherwise on the device too -- the text is uploaded once, cut at the special tokens and split into chunks by
 * mbpe_splitter_split_docs (a splitter that the tokenizer keeps until another device is named), and the encoder reads
 * that copy and its end mask in place (mbpe_encoder_encode_endmask, mbpe_encoder_encode_batch_endmask).  Same results.
 * With it set, a tokenizer whose pattern is not the built-in gpt2 or gpt4 pattern returns MBPE_ERR_ARG from those
 * calls: there is no silent return to the host split.  Nothing else is affected. */
MBPE_API int mbpe_tok_set_encode_split(mbpe_tokenizer *t, int on_device);

/* The order in which mbpe_tok_encode and the mbpe_tok_encode*_device calls apply the merges to a chunk: 0 (the
 * default) the reference's greedy passes (Tokenizer.h:325-367: a left-to-right pass replaces any pair it finds);
 * 1 rank order -- of the adjacent pairs that are in the merges, every occurrence of the one with the smallest id is
 * replaced, left to right and non-overlapping, until no pair is left.  For a trained table (both sides of merge k
 * below 256 + k, no pair twice) that replays the merges in order: the segmentation the trainer left in its stream,
 * and what other BPE implementations give for the same merges.  The host loop follows it, and the kept device encoder
 * is re-configured (mbpe_encoder_set_option "rank_order"), not re-created, with and without the device split.  Splitting
 * and special tokens are unaffected.  Any other value is MBPE_ERR_ARG. */
MBPE_API int mbpe_tok_set_encode_order(mbpe_tokenizer *t, int rank_order);

/* BPE-dropout for mbpe_tok_encode, mbpe_tok_encode_byteoff and the mbpe_tok_encode*_device calls: threshold and seed
 * as for mbpe_encoder_set_dropout (mbpe.h, which holds the definition; mbpe_dropout_threshold converts a probability).
 * The host loop applies the same instance rule -- encode_rank_ordered carries every token's byte start, with the
 * chunk's offset in its buffer as base -- and the kept device encoder is re-configured, not re-created.  A threshold
 * above 2^32 is MBPE_ERR_ARG; so is every encode call while the threshold is above 0 and the order is greedy
 * (mbpe_tok_set_encode_order): dropout is defined on the rank order alone and the order is never switched silently.
 * Positions: an instance's pos is in the coordinates of the buffer the route hands the encoder.  With the device split
 * that is the original text -- in a batch call the documents laid end to end.  With the host split, on the host loop
 * and on the device alike, it is the chunk buffer: the pattern's matches one after the other, a special token as its
 * "\0<id>" marker.  So the host loop and the device over the host split always agree, and both agree with the device
 * split whenever that buffer IS the text: no special token and no NUL-led part occurs and the pattern is basic, gpt2
 * or gpt4 (whose matches tile the text).  Otherwise the device split gives another, equally valid, draw. */
MBPE_API int mbpe_tok_set_encode_dropout(mbpe_tokenizer *t, uint64_t threshold, uint64_t seed);

/* Fill-in-the-middle for the device batch calls that pack (mbpe_tok_encode_batch_packed_device, _aux_device,
 * _windows_device and _fit_device): spec as for mbpe_encoder_set_fim (mbpe.h, which holds the rule), NULL turns it off.
 * It holds with the host split and with the device split alike; the kept device encoder is re-configured, not
 * re-created, and every other call is unaffected.  The sentinel ids may be special-token ids: the stage writes ids and
 * never looks them up.  Errors as for mbpe_encoder_set_fim; a sentinel id that does not fit a 16-bit matrix is
 * MBPE_ERR_VOCAB from the batch call.
 * mbpe_tok_encode_fim_info: mbpe_encoder_fim_info of the kept encoder -- the plan of the latest batch call; no
 * documents before the first device call. */
MBPE_API int mbpe_tok_set_encode_fim(mbpe_tokenizer *t, const mbpe_fim_spec *spec);
MBPE_API int mbpe_tok_encode_fim_info(mbpe_tokenizer *t, uint8_t *mode_out, uint64_t *cut_out, uint64_t cap_docs,
                                      uint64_t *n_docs_out);

/* Masked-LM corruption for the device batch calls that pack (those of mbpe_tok_set_encode_fim): spec as for
 * mbpe_encoder_set_mlm (mbpe.h, which holds the rule), NULL turns it off.  It holds with the host split and with the
 * device split alike; the kept device encoder is re-configured, not re-created, and every other call is unaffected.
 * The ids of the matrices are the corrupted ones and the labels of _aux_device, _windows_device and _fit_device the
 * targets (ignore_label in every cell that is none).  whole_word masks the chunks of this tokenizer's split pattern; a
 * special token is a word of its own.  mask_id and the protected ids may be special-token ids: the stage writes and
 * compares ids and never looks them up.  Errors as for mbpe_encoder_set_mlm; from the batch call MBPE_ERR_ARG while
 * fill-in-the-middle is on too and for whole_word with a 16-bit matrix, MBPE_ERR_VOCAB for a mask_id or vocab_n that
 * does not fit one. */
MBPE_API int mbpe_tok_set_encode_mlm(mbpe_tokenizer *t, const mbpe_mlm_spec *spec);

/* The option "unicode" (mbpe_splitter_set_option) of the device splits this tokenizer makes: 0 (the default) or on.
 * It applies to mbpe_tok_train_split_device and, while mbpe_tok_set_encode_split is on, to the mbpe_tok_encode*_device
 * calls, whose kept splitter is re-configured, not re-created.  Same results; otherwise without effect. */
MBPE_API int mbpe_tok_set_split_unicode(mbpe_tokenizer *t, int on);

/* Training on the distinct chunks with their counts: 0 (the default) or 1; anything else is MBPE_ERR_ARG.  While it is
 * on, mbpe_tok_train, mbpe_tok_train_split_device and mbpe_tok_train_continue split as they do (host, device,
 * mbpe_tok_set_split_unicode), then deduplicate the chunks on the device (mbpe_dedup_*, mbpe.h), load the unique
 * chunks with their counts as weights (mbpe_load_corpus_*_weighted) and train on those: the same merges, the same
 * counts, the same verbose lines, .model and .vocab, for both tie-breaks.  After the device split neither text nor mask
 * returns to the host; after the host split the packed chunks that mbpe_load_corpus_ranges would train on are
 * deduplicated, and the unique ones come back once so that the NUL rule is applied as ever.
 * The training then runs on the 32-bit loop, one merge per pass over the unique chunks.  That wins where the default
 * route takes a pass over the whole corpus per merge as well: the `first` tie-break, vocabularies beyond the 16-bit
 * slot format, a continued training.  It loses against the lexical tie-break within the slot format, which merges
 * thousands of pairs per pass.  A tokenizer without a pattern has one chunk, the whole text: it passes through the
 * deduper unhashed and trains on the 32-bit loop -- correct and slow; the route is not switched silently.
 * One rank.  A chunk above 256 bytes is never merged with its duplicates (it appears as often as it occurs). */
MBPE_API int mbpe_tok_set_train_dedup(mbpe_tokenizer *t, int on);

/* The stopping rules of the trainings from here on (mbpe_tok_train, _train_split_device, _train_continue,
 * _train_pieces_finish, with and without mbpe_tok_set_train_dedup): the context options "min_frequency" and
 * "max_token_length" of mbpe.h, 0 = off (the default).  min_frequency: 0 .. 2^31 - 1, the training ends when the best
 * pair left occurs less often; max_token_length: 0, or 2 .. 2^31 - 1 bytes, no NEW token is longer -- the merges a
 * continued training starts from stay, whatever their length.  Anything else is MBPE_ERR_ARG.  A training that ends
 * early leaves fewer than vocab_size - 256 merges, as the `first` tie-break may.  The .model and .vocab formats are
 * unchanged.
 * With either set the training runs on the 32-bit loop from its first new merge, one merge per pass over the corpus
 * it is given: combine it with mbpe_tok_set_train_dedup (or the piece-wise calls, which count words anyway), so that
 * a pass runs over the distinct chunks only.  Without dedup the result is the same and every merge is a pass over the
 * whole corpus; the route is not switched silently.  One rank; a corpus above the encoder's one-piece limit returns
 * MBPE_ERR_OOM, as for mbpe_tok_train_continue. */
MBPE_API int mbpe_tok_set_train_limits(mbpe_tokenizer *t, int64_t min_frequency, int64_t max_token_length);

/* Encoding through the distinct chunks: 0 (the default) or 1; anything else is MBPE_ERR_ARG.  While it is on,
 * mbpe_tok_encode_device and the three batch calls (mbpe_tok_encode_batch_device, _batch_packed_device,
 * _batch_aux_device) run the kept device encoder with its option "dedup" (mbpe.h: the chunks are deduplicated on the
 * device, the distinct ones go through the merge passes once, and a copy kernel writes every chunk's tokens to its
 * place), with the host split and with the device split, in both orders: the same tokens, offsets and matrices.  The
 * encoder is re-configured, not re-created.  The host loop (mbpe_tok_encode) is unaffected.  The byte-range calls on
 * a device (mbpe_tok_encode_byteoff with a device, mbpe_tok_encode_batch_byteoff_device) and every device call while
 * a dropout threshold above 0 is set return MBPE_ERR_ARG while it is on: a dropped instance depends on its position,
 * so equal chunks do not share tokens, and the route is never switched silently. */
MBPE_API int mbpe_tok_set_encode_dedup(mbpe_tokenizer *t, int on);

/* Token frequency tables: how often every token id is used on a corpus, without a token leaving the device.
 * mbpe_tok_count_tokens splits the documents as mbpe_tok_encode_batch_device does (special tokens first, each document on
 * its own) and adds what mbpe_tok_encode would return for each, `repeat` times (at least 1: 0 is MBPE_ERR_ARG), to a
 * table the tokenizer keeps on the host.
 *   device_id < 0    the host loop: mbpe_tok_encode of every document, counted
 *   device_id >= 0   the kept encoder through mbpe_encoder_count over the host split or -- after
 *                    mbpe_tok_set_encode_split(1) -- the kept splitter and mbpe_encoder_count_endmask.
 *                    mbpe_tok_set_encode_order, _dropout, _dedup and _split_unicode hold as for the batch encode calls
 *   n_tokens_out     required: the tokens of this call's documents, without repeat
 * After each device call the encoder's table is read back, added to the host's and zeroed, so an encoder that is
 * re-created (another device) loses nothing.  The table has n_ids = max(256 + n_merges, largest special id + 1)
 * entries; a special id (or 256 + n_merges) at or above MBPE_MAX_COUNT_IDS is MBPE_ERR_VOCAB before any work, and
 * MBPE_ERR_OVERFLOW comes before the weighted total could reach 2^64.  A call that fails adds nothing.  Changing the
 * merges (train, load, set_merges) or the special tokens empties the table.
 *   mbpe_tok_token_counts        counts_out (cap_ids entries; fewer than n_ids is MBPE_ERR_ARG; NULL: query), n_ids and
 *                                the weighted token total (each pointer may be NULL)
 *   mbpe_tok_token_counts_reset  empties the table */
MBPE_API int mbpe_tok_count_tokens(mbpe_tokenizer *t, const uint8_t *text, const uint64_t *doc_off, uint64_t n_docs,
                                   int verbose, int device_id, uint64_t repeat, uint64_t *n_tokens_out);
MBPE_API int mbpe_tok_token_counts(mbpe_tokenizer *t, uint64_t *counts_out, uint64_t cap_ids, uint64_t *n_ids_out,
                                   uint64_t *n_tokens_out);
MBPE_API int mbpe_tok_token_counts_reset(mbpe_tokenizer *t);

/* decode, Tokenizer.h:725-751.  bytes_out may be NULL to query the length. */
MBPE_API int mbpe_tok_decode(mbpe_tokenizer *t, const uint32_t *tokens, uint64_t n, int verbose,
                             uint8_t *bytes_out, uint64_t cap, uint64_t *n_out);

/* The same with the expansion on HIP device `device_id` (mbpe_decode_tokens, with a decoder that the tokenizer keeps
 * until its merges or special tokens change).  An id that decodes to nothing gets the reference's warning line, as
 * on the host.  No CPU fallback: MBPE_ERR_NO_DEVICE without a device. */
MBPE_API int mbpe_tok_decode_device(mbpe_tokenizer *t, const uint32_t *tokens, uint64_t n, int verbose, int device_id,
                                    uint8_t *bytes_out, uint64_t cap, uint64_t *n_out);

/* decode of n_docs documents in one device call (mbpe_decode_batch, with the same kept decoder).  Document i is
 * tokens[doc_tok_off[i] .. doc_tok_off[i + 1]): n_docs + 1 ascending offsets from 0, host memory, as
 * mbpe_tok_encode_batch_device's doc_tok_off_out; the token count is doc_tok_off[n_docs].  bytes_out (NULL: query)
 * receives the documents' texts one after the other, doc_byte_off_out (required, n_docs + 1; also on a query and
 * when cap is too small) where each begins: document i is bytes_out[doc_byte_off_out[i] .. doc_byte_off_out[i + 1])
 * and equals mbpe_tok_decode of that document's tokens.  Every id that decodes to nothing gets the reference's
 * warning line, in stream order.  The offsets are checked before a decoder is created: a bad array is MBPE_ERR_ARG
 * also where there is no device.  n_out is required; device_id must not be negative. */
MBPE_API int mbpe_tok_decode_batch_device(mbpe_tokenizer *t, const uint32_t *tokens, const uint64_t *doc_tok_off,
                                          uint64_t n_docs, int verbose, int device_id, uint8_t *bytes_out,
                                          uint64_t cap, uint64_t *doc_byte_off_out, uint64_t *n_out);

/* decode of a right-padded id matrix (host memory: n_rows x seq_len uint32_t ids, row r holding len[r] of them, as
 * MBPE_PACK_PADDED writes it without pad_left): mbpe_unpack_tokens into device memory, then one mbpe_decode_batch
 * through the kept decoder.  bytes_out, cap, doc_byte_off_out (required, n_rows + 1) and n_out as for
 * mbpe_tok_decode_batch_device, a row being a document.  A len[r] above seq_len is MBPE_ERR_ARG, also where there is
 * no device. */
MBPE_API int mbpe_tok_decode_padded_device(mbpe_tokenizer *t, const uint32_t *ids, uint64_t n_rows, uint32_t seq_len,
                                           const uint32_t *len, int verbose, int device_id, uint8_t *bytes_out,
                                           uint64_t cap, uint64_t *doc_byte_off_out, uint64_t *n_out);

#ifdef __cplusplus
}
#endif
#endif
