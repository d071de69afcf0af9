// Host-side mirror of MinBpeCC::Tokenizer::Tokenizer (reference
// code/include/Tokenizer.h:52-927): same method names, argument meaning and
// error behaviour, with train() running the lexical hot path on the GPU
// through the C-ABI of include/mbpe.h.
#ifndef MBPE_HOST_TOKENIZER_H
#define MBPE_HOST_TOKENIZER_H

#include <cstdint>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "mbpe.h"
#include "mbpe_host.h"

namespace mbpe_host {

using Token = uint32_t;                       // Tokenizer.h:38
using TokenPair = std::pair<Token, Token>;    // Tokenizer.h:40

class Tokenizer {
public:
    enum CONFLICT_RESOLUTION { FIRST, LEXICAL };   // Tokenizer.h:54-57

    Tokenizer();
    explicit Tokenizer(const std::string &pattern);   // throws std::runtime_error like :427-431
    Tokenizer(const Tokenizer &) = delete;
    Tokenizer &operator=(const Tokenizer &) = delete;
    ~Tokenizer();

    void set_special_tokens_from_file(const std::string &input_string);   // :476-486
    // :489-598; both CONFLICT_RESOLUTION values run on HIP device `device` (mbpe_train)
    // device_split: the gpt2 / gpt4 pre-split runs on the device too (mbpe_splitter_split; the text is uploaded once
    // and the trainer takes text and end mask in place).  Same merges.  A tokenizer with any other pattern throws
    // CodedError(MBPE_ERR_ARG): there is no silent return to the host split
    // resume: the tokenizer's current merges (loaded, set or trained) are the prior table of mbpe_train_begin_from: the
    // training continues from them up to vocab_size, pattern and special tokens stay, and afterwards the tokenizer holds
    // prior + new merges.  Verbose prints the per-merge line of the new merges only.  Without merges: an ordinary train
    void train(const std::string &text, int vocab_size, CONFLICT_RESOLUTION conflict_resolution, bool verbose,
               int device = 0, bool device_split = false, bool resume = false);
    // The same training on a corpus that arrives in pieces (mbpe_tok_train_pieces_*): begin opens a session on `device`
    // with a device word count (mbpe_wordcount_*); add splits a piece as train()
    // does -- on the host into packed chunks, or on the device, where neither text nor mask returns -- and counts its
    // chunks `repeat` times; finish loads the table into a fresh context (in place after the device split, through
    // mbpe_load_corpus_weighted and its NUL rule after the host split) and runs the tail of train().  The merges are
    // untouched until finish has succeeded; after finish or abort the session's device objects are gone.  Errors are
    // CodedError: MBPE_ERR_STATE for a call out of order, otherwise the code of the call that failed
    void train_pieces_begin(int device, bool device_split);
    void train_pieces_add(const char *text, uint64_t n, uint32_t repeat);
    void train_pieces_finish(int vocab_size, CONFLICT_RESOLUTION conflict_resolution, bool verbose, bool resume);
    void train_pieces_abort();
    // The open session's counts as a blob, and a blob merged into the open session (mbpe_tok_train_pieces_export /
    // _merge): the blob of mbpe_wordcount_export behind the split pattern and the chunks and bytes the session has seen,
    // so that a session which merged the blobs of all pieces finishes like one that was given all pieces.  A blob counted
    // under another pattern is CodedError(MBPE_ERR_ARG); without a session MBPE_ERR_STATE.  The session goes on
    uint64_t train_pieces_export_size();
    uint64_t train_pieces_export(uint8_t *blob_out, uint64_t cap);
    void train_pieces_merge(const uint8_t *blob, uint64_t n);
    // :653-722; device >= 0 runs internal_encode (:325-377) on that HIP device instead of the host.
    // device_split (with device >= 0, here and in the batch calls below): the text is also cut at the special tokens
    // and split into chunks on the device (mbpe_splitter_split_docs with a splitter that is kept), and the encoder
    // reads the splitter's copy of the text and its end mask in place (mbpe_encoder_encode_endmask): one upload, no
    // second buffer.  Same tokens.  A tokenizer whose pattern is not gpt2 / gpt4 throws CodedError(MBPE_ERR_ARG)
    std::vector<Token> encode(const std::string &text, bool verbose, int device = -1, bool device_split = false);
    // encode() of every text, [i] == encode(texts[i], false, -1): the chunks of all texts go to HIP device `device`
    // in one mbpe_encoder_encode, whose per-chunk token offsets are summed per text
    std::vector<std::vector<Token>> encode_batch(const std::vector<std::string> &texts, bool verbose, int device,
                                                 bool device_split = false);
    // the same over one buffer: n_docs + 1 ascending offsets.  tokens_out / cap / n_out go to mbpe_encoder_encode as
    // they are (NULL: query), whose code is returned; doc_tok_off receives n_docs + 1 token offsets when it is MBPE_OK
    int encode_batch_flat(const char *text, const uint64_t *doc_off, uint64_t n_docs, bool verbose, int device,
                          Token *tokens_out, uint64_t cap, uint64_t *n_out, uint64_t *buf_bytes_out,
                          std::vector<uint64_t> *doc_tok_off, bool device_split = false);
    // the same documents with every token's byte range: ranges[2j], ranges[2j + 1] = start and end of token j in its own
    // document's original text (a special token: the occurrence of its name).  device < 0: the host loop, ranges from
    // the vocabulary's entry lengths within each chunk; device >= 0: mbpe_encoder_encode_byteoff over the host split,
    // whose chunks carry their source ranges, or -- device_split -- mbpe_encoder_encode_endmask_byteoff, whose offsets
    // are in the documents' coordinates already.  The three agree token for token and range for range
    int encode_ranges(const char *text, const uint64_t *doc_off, uint64_t n_docs, bool verbose, int device,
                      bool device_split, std::vector<Token> *tokens, std::vector<uint64_t> *ranges,
                      std::vector<uint64_t> *doc_tok_off);
    // the same documents as one id matrix (mbpe_encoder_encode_batch; with aux, mbpe_encoder_encode_batch_aux; with
    // win, mbpe_encoder_encode_batch_windows; with fit, mbpe_encoder_encode_batch_fit): spec, ids_out .. doc_tok_off_out
    // go to it as they are, its code is returned
    int encode_batch_packed(const char *text, const uint64_t *doc_off, uint64_t n_docs, bool verbose, int device,
                            const mbpe_pack_spec *spec, void *ids_out, uint64_t cap_rows, int out_on_device,
                            uint32_t *len_out, uint64_t *n_rows_out, uint64_t *n_tokens_out,
                            const mbpe_pack_aux *aux = nullptr, uint64_t *doc_tok_off_out = nullptr,
                            bool device_split = false, const mbpe_pack_window *win = nullptr,
                            const struct mbpe_pack_fit *fit = nullptr);
    // the same documents as the two matrices of an encoder-decoder batch (mbpe_encoder_encode_batch_denoise, or --
    // device_split -- mbpe_encoder_encode_batch_endmask_denoise): the arguments go to it as they are, its code is returned
    int encode_batch_denoise(const char *text, const uint64_t *doc_off, uint64_t n_docs, bool verbose, int device,
                             const mbpe_denoise_spec *dn, const mbpe_pack_spec *enc_spec, const mbpe_pack_spec *dec_spec,
                             const mbpe_denoise_batch *out, uint64_t cap_rows, int out_on_device, uint64_t *n_rows_out,
                             uint64_t *n_tokens_out, bool device_split);
    // How often every token id is used (mbpe_tok_count_tokens): the documents are split as in encode_batch_flat and what
    // encode would return for each is counted `repeat` times into a table the tokenizer keeps on the host, of
    // count_ids() = max(256 + merges, largest special id + 1) entries.  device < 0: the host loop over encode();
    // otherwise mbpe_encoder_count over the host split or, device_split, mbpe_encoder_count_endmask over the device
    // split -- no token leaves the device; the encoder's table is read back, added and zeroed after every call.
    // Order, dropout, dedup and the unicode split hold as for the batch encode calls.  MBPE_ERR_ARG for repeat 0,
    // MBPE_ERR_VOCAB for an id at or above MBPE_MAX_COUNT_IDS, MBPE_ERR_OVERFLOW before the total could reach 2^64;
    // a call that fails adds nothing.  Changing the merges or the special tokens empties the table.  (An id beyond
    // the table can only come from a NUL-led number in the text itself; it is counted in n_tokens_out alone.)
    int count_tokens(const char *text, const uint64_t *doc_off, uint64_t n_docs, bool verbose, int device, uint64_t repeat,
                     uint64_t *n_tokens_out, bool device_split = false);
    uint64_t count_ids() const;
    const std::vector<uint64_t> &token_counts() const { return counts_; }   // empty before the first count: all zeros
    uint64_t token_counts_total() const { return counts_total_; }
    void drop_counts();
    // what the mbpe_tok_encode*_device calls of the C-ABI pass as device_split (mbpe_tok_set_encode_split)
    void set_encode_split(bool on) { encode_split_ = on; }
    bool encode_split() const { return encode_split_; }
    // the order in which encode and its batch forms apply the merges, on the host and on the device: false (the
    // default) the reference's greedy passes, true rank order (encode_rank_ordered below; mbpe_tok_set_encode_order)
    void set_rank_order(bool on) { rank_order_ = on; }
    bool rank_order() const { return rank_order_; }
    // BPE-dropout of encode and its batch forms (mbpe_tok_set_encode_dropout; dropout.h): threshold in [0, 2^32], 0 =
    // off.  With a threshold above 0 the order has to be the rank order: every encode route throws / returns
    // MBPE_ERR_ARG otherwise.  An instance's position is in the buffer the route hands the encoder: the original text
    // with the device split, the chunk buffer of append_chunks / batch_chunks with the host split (host loop and
    // device alike) -- the same whenever that buffer is the text
    void set_dropout(uint64_t threshold, uint64_t seed) { drop_threshold_ = threshold; drop_seed_ = seed; }
    // fill-in-the-middle of the device batch calls that pack (mbpe_tok_set_encode_fim; mbpe.h holds the rule): NULL =
    // off.  The kept device encoder is re-configured, not re-created; the plan of its latest batch call is its own
    // (mbpe_encoder_fim_info on kept_encoder(), NULL before the first device call)
    void set_fim(const mbpe_fim_spec *spec) { fim_on_ = spec != nullptr; if (spec) fim_ = *spec; }
    // masked-LM corruption of the same calls (mbpe_tok_set_encode_mlm; mbpe.h holds the rule): NULL = off
    void set_mlm(const mbpe_mlm_spec *spec) { mlm_on_ = spec != nullptr; if (spec) mlm_ = *spec; }
    mbpe_encoder *kept_encoder() const { return encoder_; }
    // the option "unicode" of every device split made from here on (mbpe_tok_set_split_unicode)
    void set_split_unicode(bool on) { split_unicode_ = on; }
    // train() from here on runs on the distinct chunks with their counts (mbpe_tok_set_train_dedup)
    void set_train_dedup(bool on) { train_dedup_ = on; }
    // the stopping rules of every training from here on (mbpe_tok_set_train_limits): the context options
    // "min_frequency" and "max_token_length", 0 = off
    void set_train_limits(int64_t min_frequency, int64_t max_token_length) {
        train_min_frequency_ = min_frequency;
        train_max_token_length_ = max_token_length;
    }
    // the device encode calls from here on go through the encoder's "dedup" route (mbpe_tok_set_encode_dedup)
    void set_encode_dedup(bool on) { encode_dedup_ = on; }
    // :725-751; device >= 0 expands the tokens on that HIP device (mbpe_decode_tokens) instead of the host loop
    std::string decode(const std::vector<Token> &tokens, bool verbose, int device = -1);
    // decode() of every token list, [i] == decode(docs[i], false, -1), in one mbpe_decode_batch on HIP device `device`
    std::vector<std::string> decode_batch(const std::vector<std::vector<Token>> &docs, bool verbose, int device);
    // the same over one token array: n_docs + 1 offsets that check_doc_tok_off accepts.  bytes_out / cap /
    // doc_byte_off_out / n_out go to mbpe_decode_batch as they are (NULL bytes_out: query), whose code is returned
    int decode_batch_flat(const Token *tokens, const uint64_t *doc_tok_off, uint64_t n_docs, bool verbose, int device,
                          uint8_t *bytes_out, uint64_t cap, uint64_t *doc_byte_off_out, uint64_t *n_out);
    // a right-padded matrix of n_rows x seq_len host ids with its lengths: mbpe_unpack_tokens into device memory, then
    // one mbpe_decode_batch of it as it is; row r's text is bytes_out[doc_byte_off_out[r] .. doc_byte_off_out[r + 1])
    int decode_padded(const Token *ids, uint64_t n_rows, uint32_t seq_len, const uint32_t *len, bool verbose, int device,
                      uint8_t *bytes_out, uint64_t cap, uint64_t *doc_byte_off_out, uint64_t *n_out);
    bool load(const std::string &path, bool verbose);                      // :754-872
    bool save(const std::string &path, bool write_vocab);                  // :875-926

    const std::vector<TokenPair> &get_merges() const { return merges_; }
    void set_merges(const std::vector<TokenPair> &m);
    const std::string &pattern() const { return pattern_; }

private:
    struct PairHash {
        size_t operator()(const TokenPair &k) const {          // pair_token_hash, :43-50
            size_t seed = 0;
            seed ^= std::hash<Token>()(k.first) + 0x9e3779b9 + (seed << 6) + (seed >> 2);
            seed ^= std::hash<Token>()(k.second) + 0x9e3779b9 + (seed << 6) + (seed >> 2);
            return seed;
        }
    };

    std::vector<Token> text_to_vector(const char *s, size_t n) const;       // :85-100
    void initialize_vocab();                                                // :103-111
    // :605-650; origin (optional): per part its [start, end) in text, of a marker the occurrence it replaces
    std::vector<std::string> split_on_special(const std::string &text, std::vector<uint64_t> *origin = nullptr) const;
    std::vector<Token> internal_internal_encode(std::vector<Token> text) const; // :325-367
    // the rank-ordered counterpart: of the adjacent pairs that are in merges_lookup, every occurrence of the one with
    // the smallest id is replaced, left to right and non-overlapping; repeated until no pair is left.  For a trained
    // table this replays the merges in order: the trainer's segmentation.
    // With dropout a pair whose instance (byte start of its left token, merged id) is dropped is no candidate: every
    // token carries its byte start, base = the chunk's offset in the buffer the encoder reads (off[c])
    std::vector<Token> encode_rank_ordered(std::vector<Token> text, uint64_t base) const;
    void check_dropout_order() const;      // throws CodedError(MBPE_ERR_ARG): dropout with the greedy order
    void rebuild_vocab();
    // the tail every training route shares.  training_prior: the checks of a training up to vocab_size and, with
    // resume, the merges it continues from (nothing is changed); clear_model: back to the 256 bytes; run_training: with
    // the corpus loaded into ctx (rc: the load's code, handed through when it failed) the options, the begin, the steps
    // and the result -- weights (optional): the loaded chunks' weights, with which the stream's length becomes the whole
    // corpus's; adopt_training: the vocab bookkeeping and the verbose lines
    struct Trained {
        std::vector<uint32_t> flat;
        std::vector<int32_t> had;
        uint32_t n_merges = 0;
        mbpe_stats st;
    };
    static uint32_t n_prior_of(const std::vector<uint32_t> &prior) { return static_cast<uint32_t>(prior.size() / 2); }
    std::vector<uint32_t> training_prior(int vocab_size, bool resume) const;
    void clear_model();
    int run_training(mbpe_ctx *ctx, int rc, int vocab_size, CONFLICT_RESOLUTION conflict_resolution,
                     const std::vector<uint32_t> &prior, const std::vector<uint32_t> *weights, Trained *out);
    void adopt_training(const Trained &tr, int vocab_size, uint32_t n_prior, bool verbose, uint64_t text_length);
    void drop_decoder();                   // the merges or the specials changed
    void drop_encoder();                   // the merges changed (special tokens do not enter the lookup table)
    // the chunks of n_docs texts (every text split on its own) as one buffer + offsets; first_chunk[i] = text i's first
    void batch_chunks(const char *text, const uint64_t *doc_off, uint64_t n_docs, bool verbose, std::string *buf,
                      std::vector<uint64_t> *off, std::vector<uint64_t> *first_chunk,
                      std::vector<uint64_t> *src = nullptr) const;
    // the chunks of one text appended to buf / off: special markers and, with a pattern, the regex matches of every
    // other part (:664-704); without one, every part is a chunk (:706-709)
    // src (optional): per chunk its [start, end) in text -- the part's origin plus the match, or a marker's occurrence
    void append_chunks(const std::string &text, bool verbose, std::string *buf, std::vector<uint64_t> *off,
                       std::vector<uint64_t> *src = nullptr) const;
    mbpe_encoder *device_encoder(int device);
    void drop_splitter();
    mbpe_splitter *device_splitter(int device);       // kept until another device is named or the tokenizer goes
    // the device split of n_docs texts (doc_off relative to text): the splitter's text and mask on the device, and
    // the ranges that are single tokens.  Prints the "Part:" lines of append_chunks with verbose
    struct DeviceSplit {
        const uint8_t *d_text = nullptr, *d_mask = nullptr;
        std::vector<mbpe_single> singles;
        std::vector<uint64_t> doc_off;                // rebased to 0
        uint64_t n_bytes = 0;
    };
    int split_on_device(const char *text, const uint64_t *doc_off, uint64_t n_docs, bool verbose, int device,
                        DeviceSplit *out);
    mbpe_decoder *device_decoder(int device);
    void warn_invalid(const Token *tokens, uint64_t n) const;   // the warning of :734-737 for each such id, in order

    std::string pattern_;
    Splitter splitter_;
    // the reference keeps these in unordered_maps (:64-65); insertion order is kept here so
    // that save() is deterministic
    std::vector<std::pair<std::string, Token>> special_tokens_;
    std::unordered_map<Token, std::string> special_tokens_reverse_lookup_;
    std::unordered_map<TokenPair, Token, PairHash> merges_lookup_;
    std::vector<TokenPair> merges_;
    std::vector<std::vector<Token>> vocab_;
    mbpe_decoder *decoder_ = nullptr;      // device tables of decode(..., device), kept until the model changes
    int decoder_device_ = -1;
    mbpe_encoder *encoder_ = nullptr;      // lookup table and buffers of encode(..., device), kept until the merges change
    int encoder_device_ = -1;
    mbpe_splitter *dev_splitter_ = nullptr;  // the device split of encode(..., device, device_split)
    int dev_splitter_device_ = -1;
    struct PieceSession {                    // train_pieces_*
        bool open = false, device_split = false;
        int device = 0;
        mbpe_wordcount *wc = nullptr;
        mbpe_splitter *splitter = nullptr;
        uint64_t n_chunks = 0, n_bytes = 0;  // what the verbose lines report: chunks and bytes, repeats included
    } pieces_;
    bool encode_split_ = false;
    bool split_unicode_ = false;
    bool train_dedup_ = false;
    int64_t train_min_frequency_ = 0, train_max_token_length_ = 0;
    bool encode_dedup_ = false;
    bool rank_order_ = false;
    uint64_t drop_threshold_ = 0, drop_seed_ = 0;
    bool fim_on_ = false;
    mbpe_fim_spec fim_ = {};
    bool mlm_on_ = false;
    mbpe_mlm_spec mlm_ = {};
    std::vector<uint64_t> counts_;           // count_tokens: the table, and the weighted token total it has reached
    uint64_t counts_total_ = 0;
};

}  // namespace mbpe_host

#endif
