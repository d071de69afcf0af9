// Host-side mirror of the reference Tokenizer (see tokenizer.h).  Everything
// here is host bookkeeping around the hot path: model files, special tokens,
// encode / decode.  train() hands the byte buffer and the chunk offsets to the
// GPU through mbpe_train_lexical.
#include "tokenizer.h"

#include "dropout.h"
#include "fim.h"
#include "mlm.h"
#include "mbpe.h"
#include "mbpe_tokenizer.h"

#include <cstdio>
#include <algorithm>
#include <cstring>
#include <fstream>
#include <iomanip>
#include <iostream>
#include <limits>
#include <sstream>
#include <stdexcept>

namespace mbpe_host {

Tokenizer::Tokenizer() {}

Tokenizer::~Tokenizer() {
    drop_decoder();
    drop_encoder();
    drop_splitter();
    train_pieces_abort();
}

void Tokenizer::drop_splitter() {
    if (dev_splitter_) mbpe_splitter_destroy(dev_splitter_);
    dev_splitter_ = nullptr;
    dev_splitter_device_ = -1;
}

mbpe_splitter *Tokenizer::device_splitter(int device) {
    if (!dev_splitter_ || dev_splitter_device_ != device) {
        drop_splitter();
        const int rc = mbpe_splitter_create(device, pattern_.c_str(), &dev_splitter_);
        if (rc != MBPE_OK) throw mbpe_host::CodedError(rc, mbpe_last_error());   // MBPE_ERR_ARG for a custom pattern
        dev_splitter_device_ = device;
    }
    const int rc = mbpe_splitter_set_option(dev_splitter_, "unicode", split_unicode_ ? 1 : 0);
    if (rc != MBPE_OK) throw mbpe_host::CodedError(rc, mbpe_last_error());
    return dev_splitter_;
}

void Tokenizer::drop_encoder() {
    if (encoder_) mbpe_encoder_destroy(encoder_);
    encoder_ = nullptr;
    encoder_device_ = -1;
}

mbpe_encoder *Tokenizer::device_encoder(int device) {
    if (!encoder_ || encoder_device_ != device) {
        drop_encoder();
        std::vector<uint32_t> flat;
        flat.reserve(2 * merges_.size());
        for (const auto &m : merges_) { flat.push_back(m.first); flat.push_back(m.second); }
        const int rc = mbpe_encoder_create(device, flat.data(), static_cast<uint32_t>(merges_.size()), &encoder_);
        if (rc != MBPE_OK) throw mbpe_host::CodedError(rc, mbpe_last_error());
        encoder_device_ = device;
    }
    int rc = mbpe_encoder_set_option(encoder_, "rank_order", rank_order_ ? 1 : 0);
    if (rc == MBPE_OK) rc = mbpe_encoder_set_option(encoder_, "dedup", encode_dedup_ ? 1 : 0);
    if (rc == MBPE_OK) rc = mbpe_encoder_set_dropout(encoder_, drop_threshold_, drop_seed_);
    if (rc == MBPE_OK) rc = mbpe_encoder_set_fim(encoder_, fim_on_ ? &fim_ : nullptr);
    if (rc == MBPE_OK) rc = mbpe_encoder_set_mlm(encoder_, mlm_on_ ? &mlm_ : nullptr);
    if (rc != MBPE_OK) throw mbpe_host::CodedError(rc, mbpe_last_error());
    return encoder_;
}

void Tokenizer::drop_decoder() {
    if (decoder_) mbpe_decoder_destroy(decoder_);
    decoder_ = nullptr;
    decoder_device_ = -1;
}

mbpe_decoder *Tokenizer::device_decoder(int device) {
    if (!decoder_ || decoder_device_ != device) {
        drop_decoder();
        std::vector<uint32_t> flat, ids;
        std::vector<uint64_t> off{0};
        std::string bytes;
        flat.reserve(2 * merges_.size());
        for (const auto &m : merges_) { flat.push_back(m.first); flat.push_back(m.second); }
        for (const auto &kv : special_tokens_reverse_lookup_) {
            ids.push_back(kv.first);
            bytes += kv.second;
            off.push_back(bytes.size());
        }
        const int rc = mbpe_decoder_create(device, flat.data(), static_cast<uint32_t>(merges_.size()), ids.data(),
                                           reinterpret_cast<const uint8_t *>(bytes.data()), off.data(),
                                           static_cast<uint32_t>(ids.size()), &decoder_);
        if (rc != MBPE_OK) throw mbpe_host::CodedError(rc, mbpe_last_error());
        decoder_device_ = device;
    }
    return decoder_;
}

void Tokenizer::warn_invalid(const Token *tokens, uint64_t n) const {
    for (uint64_t i = 0; i < n; ++i)
        if (tokens[i] >= vocab_.size() && !special_tokens_reverse_lookup_.count(tokens[i]))
            std::cerr << "Warning: Attempted to decode invalid token ID: " << tokens[i] << "\n";
}

Tokenizer::Tokenizer(const std::string &pattern) : pattern_(pattern) {
    std::string err;
    if (splitter_.compile(pattern, &err) != MBPE_OK) throw std::runtime_error(err);   // Tokenizer.h:427-431
}

// Tokenizer.h:85-100, with the NUL quirk :86-93 (std::stoi on the remainder).
std::vector<Token> Tokenizer::text_to_vector(const char *s, size_t n) const {
    if (n > 0 && s[0] == '\0') {
        try {
            int id = std::stoi(std::string(s + 1, n - 1));
            return std::vector<Token>{static_cast<Token>(id)};
        } catch (...) {
        }
    }
    std::vector<Token> out;
    out.reserve(n);
    for (size_t i = 0; i < n; ++i) out.push_back(static_cast<uint8_t>(s[i]));   // char_to_token :80-82
    return out;
}

void Tokenizer::initialize_vocab() {   // :103-111
    vocab_.clear();
    vocab_.reserve(256);
    for (int i = 0; i < 256; i++) vocab_.push_back(std::vector<Token>{static_cast<Token>(i)});
}

void Tokenizer::rebuild_vocab() {      // :843-861 / :562-564
    initialize_vocab();
    for (const auto &m : merges_) {
        // ids beyond the vocabulary built so far (hand-edited model) expand to nothing
        std::vector<Token> appended;
        if (m.first < vocab_.size()) appended = vocab_[m.first];
        if (m.second < vocab_.size()) appended.insert(appended.end(), vocab_[m.second].begin(), vocab_[m.second].end());
        vocab_.push_back(appended);
    }
}

void Tokenizer::set_merges(const std::vector<TokenPair> &m) {
    drop_decoder();
    drop_encoder();
    drop_counts();
    merges_ = m;
    merges_lookup_.clear();
    Token idx = 256;
    for (const auto &p : merges_) merges_lookup_[p] = idx++;   // operator[]: a repeated pair keeps the last id
    rebuild_vocab();
}

void Tokenizer::set_special_tokens_from_file(const std::string &input_string) {   // :476-486
    drop_decoder();
    drop_counts();
    special_tokens_.clear();
    special_tokens_reverse_lookup_.clear();
    std::istringstream iss(input_string);
    std::string key;
    Token value;
    while (iss >> key >> value) {
        bool found = false;
        for (auto &kv : special_tokens_)
            if (kv.first == key) { kv.second = value; found = true; }
        if (!found) special_tokens_.emplace_back(key, value);
        special_tokens_reverse_lookup_[value] = key;
    }
}

void Tokenizer::train(const std::string &text, int vocab_size, CONFLICT_RESOLUTION conflict_resolution,
                      bool verbose, int device, bool device_split, bool resume) {
    const std::vector<uint32_t> prior = training_prior(vocab_size, resume);      // (checked before anything is dropped)
    clear_model();

    const uint8_t *bytes = reinterpret_cast<const uint8_t *>(text.data());
    std::vector<uint64_t> starts, ends;
    mbpe_splitter *dev_split = nullptr;
    const uint8_t *d_text = nullptr, *d_mask = nullptr;
    if (device_split) {
        // the split on the device: one upload of the text, which the trainer then takes in place with the mask
        uint64_t n_chunks = 0;
        int rc = mbpe_splitter_create(device, pattern_.c_str(), &dev_split);
        if (rc == MBPE_OK) rc = mbpe_splitter_set_option(dev_split, "unicode", split_unicode_ ? 1 : 0);
        if (rc == MBPE_OK) rc = mbpe_splitter_split(dev_split, bytes, text.size(), 0, nullptr, nullptr, 0, &n_chunks);
        if (rc == MBPE_OK) rc = mbpe_splitter_endmask(dev_split, &d_mask, nullptr, &d_text);
        if (rc != MBPE_OK) {
            const std::string msg = mbpe_last_error();
            mbpe_splitter_destroy(dev_split);
            throw CodedError(rc, msg);
        }
        if (verbose) std::cout << "Split input text into " << n_chunks << " chunks\n";
    } else {
        std::string err;
        if (splitter_.split(bytes, text.size(), &starts, &ends, &err) != MBPE_OK) throw std::runtime_error(err);
        if (verbose) std::cout << "Split input text into " << starts.size() << " chunks\n";   // :546-548
    }
    const bool chunked = splitter_.has_pattern();

    mbpe_ctx *ctx = nullptr;
    if (mbpe_create(device, &ctx) != MBPE_OK) {
        mbpe_splitter_destroy(dev_split);
        throw std::runtime_error(mbpe_last_error());
    }
    // Dedup (mbpe_tok_set_train_dedup): the distinct chunks in order of first occurrence and their counts, and the
    // training on those with the counts as weights -- the same merges and counts, on the 32-bit loop.  After the device
    // split neither text nor mask returns to the host: the deduper reads them where the splitter left them and the
    // trainer takes the deduper's result in place.  After the host split the chunks go up packed, as
    // mbpe_load_corpus_ranges would train on them, and the unique ones come back for mbpe_load_corpus_weighted, which
    // applies the NUL rule (a custom pattern can produce such a chunk).  Without a pattern the text is one chunk:
    // nothing to deduplicate, it passes through.
    mbpe_dedup *dd = nullptr;
    std::vector<uint32_t> dd_weights;             // host copy of the weights (host split; verbose)
    int dd_rc = MBPE_OK;
    if (train_dedup_) {
        uint64_t n_unique = 0, n_unique_bytes = 0;
        dd_rc = mbpe_dedup_create(device, &dd);
        if (dd_rc == MBPE_OK && dev_split) {
            const uint8_t *u_text = nullptr, *u_mask = nullptr;
            const uint32_t *u_weights = nullptr;
            dd_rc = mbpe_dedup_chunks_endmask(dd, text.empty() ? nullptr : d_text, text.size(), text.empty() ? nullptr : d_mask,
                                              &n_unique, &n_unique_bytes);
            if (dd_rc == MBPE_OK) dd_rc = mbpe_dedup_result(dd, &u_text, &u_mask, &u_weights, nullptr);
            if (dd_rc == MBPE_OK)
                dd_rc = mbpe_load_corpus_endmask_weighted(ctx, u_text, n_unique_bytes, 1, u_mask, u_weights, n_unique, 1);
            if (dd_rc == MBPE_OK && verbose) {
                dd_weights.resize(n_unique);
                dd_rc = mbpe_dedup_get(dd, nullptr, nullptr, dd_weights.data(), nullptr, 0, n_unique);
            }
        } else if (dd_rc == MBPE_OK) {
            std::string packed;
            std::vector<uint64_t> off(1, 0);
            if (chunked) {
                for (size_t i = 0; i < starts.size(); ++i) {
                    packed.append(text, starts[i], ends[i] - starts[i]);
                    off.push_back(packed.size());
                }
            } else {
                off.push_back(text.size());
            }
            const std::string &src = chunked ? packed : text;
            dd_rc = mbpe_dedup_chunks(dd, reinterpret_cast<const uint8_t *>(src.data()), src.size(), 0, off.data(),
                                      off.size() - 1, &n_unique, &n_unique_bytes);
            std::vector<uint8_t> u_text(n_unique_bytes + 1);
            std::vector<uint64_t> u_off(n_unique + 1, 0);
            dd_weights.resize(n_unique);
            if (dd_rc == MBPE_OK)
                dd_rc = mbpe_dedup_get(dd, u_text.data(), u_off.data(), dd_weights.data(), nullptr, n_unique_bytes, n_unique);
            if (dd_rc == MBPE_OK)
                dd_rc = mbpe_load_corpus_weighted(ctx, u_text.data(), n_unique_bytes, u_off.data(), n_unique, 0,
                                                  dd_weights.data());
        }
    }
    // chunks as ranges: bytes between two matches belong to no chunk, as in the reference's loop (:506-540).  The
    // device split's mask goes to the trainer as it is: the NUL rule of text_to_vector (:86-93) never fires for the
    // gpt2 / gpt4 patterns -- a chunk that starts with NUL holds no ASCII digit, so std::stoi cannot parse its remainder
    int rc = train_dedup_ ? dd_rc
             : dev_split  ? mbpe_load_corpus_endmask(ctx, text.empty() ? bytes : d_text, text.size(), !text.empty(), d_mask)
             : chunked    ? mbpe_load_corpus_ranges(ctx, bytes, text.size(), starts.data(), ends.data(), starts.size(), 0)
                          : mbpe_load_corpus(ctx, bytes, text.size(), nullptr, 0, 0);
    Trained tr;
    rc = run_training(ctx, rc, vocab_size, conflict_resolution, prior, train_dedup_ && verbose ? &dd_weights : nullptr, &tr);
    std::string msg = rc == MBPE_OK ? "" : mbpe_last_error();
    mbpe_destroy(ctx);
    mbpe_dedup_destroy(dd);                 // (the trainer has its own copies of mask and weights; the text until here)
    mbpe_splitter_destroy(dev_split);       // (its text and mask were in use until here)
    if (rc != MBPE_OK && resume) throw CodedError(rc, msg);      // (mbpe_tok_train_continue hands the code on)
    if (rc != MBPE_OK) throw std::runtime_error(msg);
    adopt_training(tr, vocab_size, n_prior_of(prior), verbose, text.length());
}

std::vector<uint32_t> Tokenizer::training_prior(int vocab_size, bool resume) const {
    if (vocab_size < 256) throw std::runtime_error("vocab_size must be >= 256");   // assert, :492
    // the table a resumed training continues from: what the tokenizer holds
    std::vector<uint32_t> prior;
    if (resume) {
        for (const TokenPair &mp : merges_) { prior.push_back(mp.first); prior.push_back(mp.second); }
        if (prior.size() / 2 > static_cast<size_t>(vocab_size - 256))
            throw CodedError(MBPE_ERR_ARG, "vocab_size " + std::to_string(vocab_size) + " is below the " +
                                               std::to_string(256 + prior.size() / 2) + " tokens the model already has");
        if (mbpe_merges_check(prior.data(), static_cast<uint32_t>(prior.size() / 2)) != MBPE_OK)
            throw CodedError(MBPE_ERR_ARG, mbpe_last_error());
    }
    return prior;
}

void Tokenizer::clear_model() {
    drop_decoder();
    drop_encoder();
    drop_counts();
    merges_.clear();
    merges_lookup_.clear();
    initialize_vocab();
}

int Tokenizer::run_training(mbpe_ctx *ctx, int rc, int vocab_size, CONFLICT_RESOLUTION conflict_resolution,
                            const std::vector<uint32_t> &prior, const std::vector<uint32_t> *weights, Trained *out) {
    const uint32_t cap = static_cast<uint32_t>(vocab_size - 256);
    out->flat.assign(2 * static_cast<size_t>(cap) + 2, 0);
    out->had.assign(cap + 1, 0);
    out->n_merges = 0;
    mbpe_stats &st = out->st;
    if (rc == MBPE_OK) rc = mbpe_set_option(ctx, "conflict_resolution", conflict_resolution == LEXICAL ? 1 : 0);
    // (`first` beyond the 16-bit slot format continues on 32-bit tokens, as the reference's uint32_t Token does)
    if (rc == MBPE_OK) rc = mbpe_set_option(ctx, "first_wide", 1);
    // (... and so does a training that continues from existing merges)
    if (rc == MBPE_OK) rc = mbpe_set_option(ctx, "resume_wide", 1);
    // (the stopping rules, mbpe_tok_set_train_limits: either non-zero and the training runs on 32-bit tokens throughout)
    if (rc == MBPE_OK) rc = mbpe_set_option(ctx, "min_frequency", train_min_frequency_);
    if (rc == MBPE_OK) rc = mbpe_set_option(ctx, "max_token_length", train_max_token_length_);
    if (rc == MBPE_OK) rc = mbpe_train_begin_from(ctx, static_cast<uint32_t>(vocab_size), prior.data(), n_prior_of(prior));
    if (rc == MBPE_OK) rc = mbpe_train_steps(ctx, cap, nullptr);
    if (rc == MBPE_OK) rc = mbpe_train_result(ctx, out->flat.data(), out->had.data(), cap, &out->n_merges);
    if (rc == MBPE_OK) rc = mbpe_get_stats(ctx, &st);
    if (rc == MBPE_OK && weights) {
        // the length the verbose line reports is the full corpus's: every unique chunk's tokens, weights[c] times
        uint64_t n_stream = 0;
        rc = mbpe_get_stream(ctx, nullptr, nullptr, 0, &n_stream);
        std::vector<uint32_t> toks(n_stream + 1);
        std::vector<uint8_t> is_end(n_stream + 1);
        if (rc == MBPE_OK) rc = mbpe_get_stream(ctx, toks.data(), is_end.data(), n_stream, &n_stream);
        uint64_t total = 0, chunk = 0;
        for (uint64_t i = 0; i < n_stream && rc == MBPE_OK; ++i) {
            total += chunk < weights->size() ? (*weights)[chunk] : 1;
            if (is_end[i]) ++chunk;
        }
        st.n_live = total;
    }
    return rc;
}

void Tokenizer::adopt_training(const Trained &tr, int vocab_size, uint32_t n_prior, bool verbose, uint64_t text_length) {
    const int total_merges = vocab_size - 256;
    for (uint32_t k = 0; k < tr.n_merges; ++k) {         // the bookkeeping of :562-579
        const TokenPair mp{tr.flat[2 * k], tr.flat[2 * k + 1]};
        std::vector<Token> appended{vocab_[mp.first]};
        appended.insert(appended.end(), vocab_[mp.second].begin(), vocab_[mp.second].end());
        vocab_.push_back(appended);
        if (verbose && k >= n_prior) {                   // :565-577 (a resumed training: the new merges)
            std::string s;
            for (auto c : appended) s += (c >= 32 && c < 127) ? static_cast<char>(c) : ' ';
            std::cout << "merge " << k + 1 << "/" << total_merges << ": (" << mp.first << ", " << mp.second
                      << ") -> " << 256 + k << " (b'" << s << "') had " << tr.had[k] << " occurrences\n";
        }
        merges_.push_back(mp);
        merges_lookup_[mp] = 256 + k;
    }
    if (verbose)                                         // :591-597
        std::cout << "Length of training text " << text_length << ". After merges " << tr.st.n_live << ".\n";
}

// ---- training on a corpus that arrives in pieces (mbpe_tok_train_pieces_*) ---------------------------------------------
void Tokenizer::train_pieces_abort() {
    if (pieces_.wc) mbpe_wordcount_destroy(pieces_.wc);
    if (pieces_.splitter) mbpe_splitter_destroy(pieces_.splitter);
    pieces_ = PieceSession();
}

void Tokenizer::train_pieces_begin(int device, bool device_split) {
    if (pieces_.open) throw CodedError(MBPE_ERR_STATE, "train_pieces_begin: a session is open already");
    PieceSession s;
    s.device = device;
    s.device_split = device_split;
    const int rc = mbpe_wordcount_create(device, &s.wc);
    if (rc != MBPE_OK) throw CodedError(rc, mbpe_last_error());
    s.open = true;
    pieces_ = s;
}

void Tokenizer::train_pieces_add(const char *text, uint64_t n, uint32_t repeat) {
    if (!pieces_.open) throw CodedError(MBPE_ERR_STATE, "train_pieces_add: no session is open (train_pieces_begin)");
    if (repeat == 0) throw CodedError(MBPE_ERR_ARG, "train_pieces_add: repeat must be at least 1");
    static const char nothing = 0;
    if (!text) text = &nothing;                   // (an empty piece)
    const uint8_t *bytes = reinterpret_cast<const uint8_t *>(text);
    uint64_t n_chunks = 0, n_unique = 0;
    int rc;
    if (pieces_.device_split) {
        // split and counted on the device: neither the text nor its mask returns to the host
        // (one splitter for the session; a custom pattern is refused: MBPE_ERR_ARG, no return to the host split)
        const uint8_t *d_text = nullptr, *d_mask = nullptr;
        rc = pieces_.splitter ? MBPE_OK : mbpe_splitter_create(pieces_.device, pattern_.c_str(), &pieces_.splitter);
        if (rc == MBPE_OK) rc = mbpe_splitter_set_option(pieces_.splitter, "unicode", split_unicode_ ? 1 : 0);
        if (rc == MBPE_OK) rc = mbpe_splitter_split(pieces_.splitter, bytes, n, 0, nullptr, nullptr, 0, &n_chunks);
        if (rc == MBPE_OK) rc = mbpe_splitter_endmask(pieces_.splitter, &d_mask, nullptr, &d_text);
        if (rc == MBPE_OK)
            rc = mbpe_wordcount_add_endmask(pieces_.wc, n ? d_text : nullptr, n, n ? d_mask : nullptr, repeat, &n_unique,
                                            nullptr);
    } else {
        // the chunks packed, as Tokenizer::train hands them to the deduper; without a pattern the piece is one chunk
        std::vector<uint64_t> off(1, 0);
        std::string packed;
        const bool chunked = splitter_.has_pattern();
        if (chunked) {
            std::vector<uint64_t> starts, ends;
            std::string err;
            if (splitter_.split(bytes, n, &starts, &ends, &err) != MBPE_OK) throw std::runtime_error(err);
            for (size_t i = 0; i < starts.size(); ++i) {
                packed.append(text + starts[i], ends[i] - starts[i]);
                off.push_back(packed.size());
            }
        } else {
            off.push_back(n);
        }
        n_chunks = off.size() - 1;
        rc = mbpe_wordcount_add(pieces_.wc, chunked ? reinterpret_cast<const uint8_t *>(packed.data()) : bytes,
                                chunked ? packed.size() : n, 0, off.data(), n_chunks, repeat, &n_unique, nullptr);
    }
    if (rc != MBPE_OK) throw CodedError(rc, mbpe_last_error());
    pieces_.n_chunks += n_chunks * repeat;
    pieces_.n_bytes += n * repeat;
}

// The session's counts as a blob: 32 bytes -- u32 magic "MBTC", u32 version, u64 length of the split pattern, u64 chunks
// and u64 bytes the session has seen (what the verbose lines of finish report) -- then the pattern padded with zeros to
// 8 bytes, then the blob of mbpe_wordcount_export.  Little-endian, as the hosts this runs on.
namespace {
constexpr uint32_t kCountsMagic = 0x4354424Du, kCountsVersion = 1;        // "MBTC"
constexpr uint64_t kCountsHeader = 32;
uint64_t counts_prefix(uint64_t pattern_len) { return kCountsHeader + (pattern_len + 7) / 8 * 8; }
}  // namespace

uint64_t Tokenizer::train_pieces_export_size() {
    if (!pieces_.open) throw CodedError(MBPE_ERR_STATE, "train_pieces_export: no session is open (train_pieces_begin)");
    uint64_t n = 0;
    const int rc = mbpe_wordcount_export_size(pieces_.wc, &n);
    if (rc != MBPE_OK) throw CodedError(rc, mbpe_last_error());
    return counts_prefix(pattern_.size()) + n;
}

uint64_t Tokenizer::train_pieces_export(uint8_t *blob_out, uint64_t cap) {
    const uint64_t size = train_pieces_export_size(), prefix = counts_prefix(pattern_.size());
    if (cap < size) throw CodedError(MBPE_ERR_ARG, "train_pieces_export: blob_out is too small");
    const uint32_t head[2] = {kCountsMagic, kCountsVersion};
    const uint64_t fields[3] = {pattern_.size(), pieces_.n_chunks, pieces_.n_bytes};
    memset(blob_out, 0, prefix);
    memcpy(blob_out, head, 8);
    memcpy(blob_out + 8, fields, 24);
    memcpy(blob_out + kCountsHeader, pattern_.data(), pattern_.size());
    const int rc = mbpe_wordcount_export(pieces_.wc, blob_out + prefix, cap - prefix, nullptr);
    if (rc != MBPE_OK) throw CodedError(rc, mbpe_last_error());
    return size;
}

void Tokenizer::train_pieces_merge(const uint8_t *blob, uint64_t n) {
    if (!pieces_.open) throw CodedError(MBPE_ERR_STATE, "train_pieces_merge: no session is open (train_pieces_begin)");
    uint32_t head[2] = {0, 0};
    uint64_t fields[3] = {0, 0, 0};
    if (n >= kCountsHeader) {
        memcpy(head, blob, 8);
        memcpy(fields, blob + 8, 24);
    }
    if (n < kCountsHeader || head[0] != kCountsMagic || head[1] != kCountsVersion || fields[0] > n - kCountsHeader ||
        counts_prefix(fields[0]) > n)
        throw CodedError(MBPE_ERR_ARG, "train_pieces_merge: not a counts blob (truncated, bad magic or unknown version)");
    if (fields[0] != pattern_.size() || memcmp(blob + kCountsHeader, pattern_.data(), pattern_.size()) != 0)
        throw CodedError(MBPE_ERR_ARG, "train_pieces_merge: the blob was counted under another split pattern");
    const uint64_t prefix = counts_prefix(fields[0]);
    const int rc = mbpe_wordcount_merge_blob(pieces_.wc, blob + prefix, n - prefix, nullptr, nullptr);
    if (rc != MBPE_OK) throw CodedError(rc, mbpe_last_error());
    pieces_.n_chunks += fields[1];
    pieces_.n_bytes += fields[2];
}

void Tokenizer::train_pieces_finish(int vocab_size, CONFLICT_RESOLUTION conflict_resolution, bool verbose, bool resume) {
    if (!pieces_.open) throw CodedError(MBPE_ERR_STATE, "train_pieces_finish: no session is open (train_pieces_begin)");
    // the session ends here, however this goes; the merges stay as they are until the training has succeeded
    struct Close {
        Tokenizer *t;
        ~Close() { t->train_pieces_abort(); }
    } close{this};
    const std::vector<uint32_t> prior = training_prior(vocab_size, resume);
    if (verbose) std::cout << "Split input text into " << pieces_.n_chunks << " chunks\n";
    uint64_t n_unique = 0, n_unique_bytes = 0;
    int rc = mbpe_wordcount_stats(pieces_.wc, nullptr, nullptr, &n_unique, &n_unique_bytes);
    mbpe_ctx *ctx = nullptr;
    if (rc == MBPE_OK) rc = mbpe_create(pieces_.device, &ctx);
    std::vector<uint32_t> weights(n_unique);
    if (rc == MBPE_OK && pieces_.device_split) {
        // the table is loaded where it lies
        const uint8_t *u_text = nullptr, *u_mask = nullptr;
        const uint32_t *u_weights = nullptr;
        rc = mbpe_wordcount_result(pieces_.wc, &u_text, &u_mask, &u_weights, nullptr);
        if (rc == MBPE_OK)
            rc = mbpe_load_corpus_endmask_weighted(ctx, u_text, n_unique_bytes, 1, u_mask, u_weights, n_unique, 1);
        if (rc == MBPE_OK && verbose)
            rc = mbpe_wordcount_get(pieces_.wc, nullptr, nullptr, weights.data(), nullptr, 0, n_unique);
    } else if (rc == MBPE_OK) {
        // the unique chunks come back once, so that the NUL rule is applied as ever
        std::vector<uint8_t> u_text(n_unique_bytes + 1);
        std::vector<uint64_t> u_off(n_unique + 1, 0);
        rc = mbpe_wordcount_get(pieces_.wc, u_text.data(), u_off.data(), weights.data(), nullptr, n_unique_bytes, n_unique);
        if (rc == MBPE_OK)
            rc = mbpe_load_corpus_weighted(ctx, u_text.data(), n_unique_bytes, u_off.data(), n_unique, 0, weights.data());
    }
    Trained tr;
    rc = run_training(ctx, rc, vocab_size, conflict_resolution, prior, verbose ? &weights : nullptr, &tr);
    const std::string msg = rc == MBPE_OK ? "" : mbpe_last_error();
    if (ctx) mbpe_destroy(ctx);             // (the table's text was in use until here)
    if (rc != MBPE_OK) throw CodedError(rc, msg);
    const uint64_t n_bytes = pieces_.n_bytes;
    clear_model();
    adopt_training(tr, vocab_size, n_prior_of(prior), verbose, n_bytes);
}

// :605-650
// :605-650.  Same result as the reference's rescan-from-the-cursor loop, computed in one sweep: every occurrence of
// every special token is listed once, sorted by (position, token order), and an occurrence is taken when it starts
// at or after the end of the previous one taken.  A taken token becomes the marker "\0<id>" (:635-637).
std::vector<std::string> Tokenizer::split_on_special(const std::string &text, std::vector<uint64_t> *origin) const {
    std::vector<std::string> parts;
    // origin (optional): per part its [start, end) in text -- of a marker, the occurrence of the name it replaces
    auto from = [&](size_t s, size_t e) { if (origin) { origin->push_back(s); origin->push_back(e); } };
    struct Occ { size_t pos; size_t tok; };
    std::vector<Occ> occ;
    for (size_t k = 0; k < special_tokens_.size(); ++k) {
        const std::string &name = special_tokens_[k].first;
        if (name.empty()) continue;
        for (size_t p = text.find(name); p != std::string::npos; p = text.find(name, p + 1)) occ.push_back({p, k});
    }
    std::sort(occ.begin(), occ.end(), [](const Occ &a, const Occ &b) { return a.pos != b.pos ? a.pos < b.pos : a.tok < b.tok; });
    size_t cursor = 0;
    for (const Occ &o : occ) {
        if (o.pos < cursor) continue;                      // inside a token already taken
        if (o.pos > cursor) { parts.push_back(text.substr(cursor, o.pos - cursor)); from(cursor, o.pos); }
        parts.push_back(std::string(1, '\0') + std::to_string(special_tokens_[o.tok].second));
        cursor = o.pos + special_tokens_[o.tok].first.size();
        from(o.pos, cursor);
    }
    if (cursor < text.size()) { parts.push_back(text.substr(cursor)); from(cursor, text.size()); }
    if (parts.empty()) { parts.push_back(text); from(0, text.size()); }
    return parts;
}

// :325-367: one left-to-right pass replacing ANY pair found in merges_lookup
// (first match wins, not rank order), repeated until a pass changes nothing.
std::vector<Token> Tokenizer::internal_internal_encode(std::vector<Token> text) const {
    for (;;) {
        if (text.size() < 2) return text;
        std::vector<Token> out;
        out.reserve(text.size());
        size_t i = 0, merge_count = 0;
        const size_t len = text.size();
        while (i < len) {
            bool merged = false;
            if (i + 1 < len) {
                auto it = merges_lookup_.find(TokenPair{text[i], text[i + 1]});
                if (it != merges_lookup_.end()) {
                    out.push_back(it->second);
                    i += 2;
                    merge_count++;
                    merged = true;
                }
            }
            if (!merged) out.push_back(text[i++]);
        }
        if (merge_count == 0) return out;
        text.swap(out);
    }
}

void Tokenizer::check_dropout_order() const {
    if (drop_threshold_ && !rank_order_)
        throw CodedError(MBPE_ERR_ARG, "encode: dropout needs the rank order (mbpe_tok_set_encode_order)");
}

std::vector<Token> Tokenizer::encode_rank_ordered(std::vector<Token> text, uint64_t base) const {
    const bool drop = drop_threshold_ != 0;
    std::vector<uint64_t> pos, pos_out;            // dropout only: the byte start of every token
    if (drop) {
        pos.resize(text.size());
        for (size_t i = 0; i < text.size(); ++i) pos[i] = base + i;      // (text_to_vector: one token per byte, or one)
    }
    // the id (t[i], t[i + 1]) merges to when the pair is in the lookup and its instance survives, else "none"
    const Token none = std::numeric_limits<Token>::max();
    auto candidate = [&](size_t i) -> Token {
        auto it = merges_lookup_.find(TokenPair{text[i], text[i + 1]});
        if (it == merges_lookup_.end()) return none;
        if (drop && mbpe::dropout_dropped(drop_seed_, pos[i], it->second, drop_threshold_)) return none;
        return it->second;
    };
    for (;;) {
        Token best = none;
        for (size_t i = 0; i + 1 < text.size(); ++i) best = std::min(best, candidate(i));
        if (best == none) return text;
        std::vector<Token> out;
        out.reserve(text.size());
        pos_out.clear();
        for (size_t i = 0; i < text.size();) {
            const bool hit = i + 1 < text.size() && candidate(i) == best;
            out.push_back(hit ? best : text[i]);
            if (drop) pos_out.push_back(pos[i]);
            i += hit ? 2 : 1;
        }
        text.swap(out);
        pos.swap(pos_out);
    }
}

void Tokenizer::append_chunks(const std::string &text, bool verbose, std::string *buf, std::vector<uint64_t> *off,
                              std::vector<uint64_t> *src) const {
    std::vector<uint64_t> origin;
    auto split_text = split_on_special(text, src ? &origin : nullptr);
    if (verbose) {
        std::cout << "Splitting input text into " << split_text.size() << " parts\n";
        for (const auto &part : split_text) {
            bool is_special = part.size() > 0 && part[0] == '\0';
            std::cout << "Part: \"" << part << "\" special: " << is_special << "\n";
        }
    }
    for (size_t k = 0; k < split_text.size(); ++k) {
        const std::string &part = split_text[k];
        if (splitter_.has_pattern() && !(part.size() > 0 && part[0] == '\0')) {
            std::vector<uint64_t> starts, ends;
            std::string err;
            if (splitter_.split(reinterpret_cast<const uint8_t *>(part.data()), part.size(), &starts, &ends, &err) !=
                MBPE_OK)
                throw std::runtime_error(err);                   // :686-691
            for (size_t i = 0; i < starts.size(); ++i) {
                buf->append(part, starts[i], ends[i] - starts[i]);
                off->push_back(buf->size());
                if (src) { src->push_back(origin[2 * k] + starts[i]); src->push_back(origin[2 * k] + ends[i]); }
            }
        } else {
            *buf += part;
            off->push_back(buf->size());
            if (src) { src->push_back(origin[2 * k]); src->push_back(origin[2 * k + 1]); }
        }
    }
}

int Tokenizer::split_on_device(const char *text, const uint64_t *doc_off, uint64_t n_docs, bool verbose, int device,
                               DeviceSplit *out) {
    mbpe_splitter *sp = device_splitter(device);
    const uint64_t base = n_docs ? doc_off[0] : 0;
    out->doc_off.resize(n_docs + 1);
    for (uint64_t i = 0; i <= n_docs; ++i) out->doc_off[i] = n_docs ? doc_off[i] - base : 0;
    out->n_bytes = out->doc_off[n_docs];
    const char *t = text + base;
    std::string names;
    std::vector<uint64_t> name_off{0};
    for (const auto &kv : special_tokens_) {
        names += kv.first;
        name_off.push_back(names.size());
    }
    uint64_t n_chunks = 0, n_ranges = 0;
    int rc = mbpe_splitter_split_docs(sp, reinterpret_cast<const uint8_t *>(t), out->n_bytes, 0, out->doc_off.data(), n_docs,
                                      reinterpret_cast<const uint8_t *>(names.data()), name_off.data(),
                                      static_cast<uint32_t>(special_tokens_.size()), nullptr, nullptr, 0, &n_ranges,
                                      &n_chunks);
    if (rc != MBPE_OK) return rc;
    const mbpe_split_range *ranges = nullptr;
    rc = mbpe_splitter_ranges(sp, &ranges, &n_ranges);
    if (rc == MBPE_OK) rc = mbpe_splitter_endmask(sp, &out->d_mask, nullptr, &out->d_text);
    if (rc != MBPE_OK) return rc;
    // a taken occurrence is its special id; a NUL-led part is one token when std::stoi parses its remainder (:86-93)
    out->singles.clear();
    for (uint64_t k = 0; k < n_ranges; ++k) {
        const mbpe_split_range &r = ranges[k];
        if (r.name != MBPE_SPLIT_RAW) {
            out->singles.push_back({r.start, r.len, special_tokens_[r.name].second, 0});
            continue;
        }
        try {
            const int id = std::stoi(std::string(t + r.start + 1, r.len - 1));
            out->singles.push_back({r.start, r.len, static_cast<Token>(id), 0});
        } catch (...) {                                          // stays bytes, as one chunk
        }
    }
    if (verbose) {                                               // the lines of append_chunks, document by document
        uint64_t k = 0;
        for (uint64_t d = 0; d < n_docs; ++d) {
            const uint64_t s = out->doc_off[d], e = out->doc_off[d + 1];
            if (e == s) continue;
            std::vector<std::string> parts;
            uint64_t cursor = s;
            for (; k < n_ranges && ranges[k].start < e; ++k) {
                if (ranges[k].name == MBPE_SPLIT_RAW) continue;  // (a part like any other: printed as the text it is)
                if (ranges[k].start > cursor) parts.push_back(std::string(t + cursor, ranges[k].start - cursor));
                parts.push_back(std::string(1, '\0') + std::to_string(special_tokens_[ranges[k].name].second));
                cursor = ranges[k].start + ranges[k].len;
            }
            if (cursor < e) parts.push_back(std::string(t + cursor, e - cursor));
            std::cout << "Splitting input text into " << parts.size() << " parts\n";
            for (const auto &part : parts) {
                bool is_special = part.size() > 0 && part[0] == '\0';
                std::cout << "Part: \"" << part << "\" special: " << is_special << "\n";
            }
        }
    }
    return MBPE_OK;
}

// :653-722.  device < 0: internal_encode on the host (below); device >= 0: on that HIP device (mbpe_encoder_encode,
// with an encoder that is kept until the merges change)
std::vector<Token> Tokenizer::encode(const std::string &text, bool verbose, int device, bool device_split) {
    check_dropout_order();
    if (device >= 0 && device_split) {
        const uint64_t doc_off[2] = {0, text.size()};
        DeviceSplit ds;
        int rc = split_on_device(text.data(), doc_off, 1, verbose, device, &ds);
        if (rc != MBPE_OK) throw mbpe_host::CodedError(rc, mbpe_last_error());
        mbpe_encoder *enc = device_encoder(device);
        std::vector<Token> out(text.size());
        uint64_t n = 0;
        rc = mbpe_encoder_encode_endmask(enc, ds.d_text, text.size(), ds.d_mask, ds.singles.data(), ds.singles.size(),
                                         nullptr, 0, out.data(), out.size(), 32, 0, nullptr, &n, nullptr);
        if (rc != MBPE_OK) throw mbpe_host::CodedError(rc, mbpe_last_error());
        out.resize(n);
        if (verbose) std::cout << "Encoded input text (length " << text.length() << ") to " << out.size() << " tokens\n";
        return out;
    }
    // the chunks, as one byte buffer + offsets
    std::string buf;
    std::vector<uint64_t> off{0};
    buf.reserve(text.size() + 64);
    append_chunks(text, verbose, &buf, &off);
    std::vector<Token> out;
    if (device >= 0) {
        mbpe_encoder *enc = device_encoder(device);
        out.resize(buf.size());
        uint64_t n = 0;
        const int rc = mbpe_encoder_encode(enc, reinterpret_cast<const uint8_t *>(buf.data()), buf.size(), 0, off.data(),
                                           off.size() - 1, out.data(), out.size(), 32, 0, nullptr, &n, nullptr);
        if (rc != MBPE_OK) throw mbpe_host::CodedError(rc, mbpe_last_error());       // (the C-ABI hands the code on unchanged)
        out.resize(n);
    } else {
        for (size_t c = 0; c + 1 < off.size(); ++c) {           // internal_encode :370-377 + flatten :713-717
            auto vec = text_to_vector(buf.data() + off[c], off[c + 1] - off[c]);
            auto enc = rank_order_ ? encode_rank_ordered(std::move(vec), off[c]) : internal_internal_encode(std::move(vec));
            out.insert(out.end(), enc.begin(), enc.end());
        }
    }
    if (verbose) std::cout << "Encoded input text (length " << text.length() << ") to " << out.size() << " tokens\n";
    return out;
}

void Tokenizer::batch_chunks(const char *text, const uint64_t *doc_off, uint64_t n_docs, bool verbose, std::string *buf,
                             std::vector<uint64_t> *off, std::vector<uint64_t> *first_chunk,
                             std::vector<uint64_t> *src) const {
    // every text is split on its own (a chunk never spans two texts)
    off->assign(1, 0);
    first_chunk->assign(n_docs + 1, 0);
    buf->reserve(doc_off[n_docs] - doc_off[0] + 64);
    for (uint64_t i = 0; i < n_docs; ++i) {
        (*first_chunk)[i] = off->size() - 1;
        if (doc_off[i + 1] > doc_off[i])                          // (an empty text has no chunk: an empty result)
            append_chunks(std::string(text + doc_off[i], doc_off[i + 1] - doc_off[i]), verbose, buf, off, src);
    }
    (*first_chunk)[n_docs] = off->size() - 1;
}

int Tokenizer::encode_batch_flat(const char *text, const uint64_t *doc_off, uint64_t n_docs, bool verbose, int device,
                                 Token *tokens_out, uint64_t cap, uint64_t *n_out, uint64_t *buf_bytes_out,
                                 std::vector<uint64_t> *doc_tok_off, bool device_split) {
    if (device_split) {
        DeviceSplit ds;
        int rc = split_on_device(text, doc_off, n_docs, verbose, device, &ds);
        if (rc != MBPE_OK) return rc;
        if (buf_bytes_out) *buf_bytes_out = ds.n_bytes;
        mbpe_encoder *enc = device_encoder(device);
        std::vector<uint64_t> tok_off(n_docs + 1, 0);
        rc = mbpe_encoder_encode_endmask(enc, ds.d_text, ds.n_bytes, ds.d_mask, ds.singles.data(), ds.singles.size(),
                                         ds.doc_off.data(), n_docs, tokens_out, cap, 32, 0, tok_off.data(), n_out, nullptr);
        if (rc != MBPE_OK) return rc;
        doc_tok_off->swap(tok_off);
        if (verbose) std::cout << "Encoded " << n_docs << " texts (length " << ds.n_bytes << ") to " << *n_out << " tokens\n";
        return MBPE_OK;
    }
    std::string buf;
    std::vector<uint64_t> off, first_chunk;
    batch_chunks(text, doc_off, n_docs, verbose, &buf, &off, &first_chunk);
    if (buf_bytes_out) *buf_bytes_out = buf.size();
    mbpe_encoder *enc = device_encoder(device);
    std::vector<uint64_t> chunk_tok_off(off.size(), 0);
    const int rc = mbpe_encoder_encode(enc, reinterpret_cast<const uint8_t *>(buf.data()), buf.size(), 0, off.data(),
                                       off.size() - 1, tokens_out, cap, 32, 0, chunk_tok_off.data(), n_out, nullptr);
    if (rc != MBPE_OK) return rc;
    doc_tok_off->resize(n_docs + 1);
    for (uint64_t i = 0; i <= n_docs; ++i) (*doc_tok_off)[i] = chunk_tok_off[first_chunk[i]];
    if (verbose) std::cout << "Encoded " << n_docs << " texts (length " << buf.size() << ") to " << *n_out << " tokens\n";
    return MBPE_OK;
}

void Tokenizer::drop_counts() {
    counts_.clear();
    counts_total_ = 0;
}

uint64_t Tokenizer::count_ids() const {
    uint64_t n = 256 + static_cast<uint64_t>(merges_.size());
    for (const auto &kv : special_tokens_) n = std::max<uint64_t>(n, static_cast<uint64_t>(kv.second) + 1);
    return n;
}

int Tokenizer::count_tokens(const char *text, const uint64_t *doc_off, uint64_t n_docs, bool verbose, int device,
                            uint64_t repeat, uint64_t *n_tokens_out, bool device_split) {
    *n_tokens_out = 0;
    auto fail = [](int code, const std::string &msg) { mbpe_host::set_last_error(msg); return code; };
    if (repeat == 0) return fail(MBPE_ERR_ARG, "count_tokens: repeat must be at least 1");
    const uint64_t n_ids = count_ids();
    if (n_ids > MBPE_MAX_COUNT_IDS) return fail(MBPE_ERR_VOCAB, "count_tokens: a token id at or above MBPE_MAX_COUNT_IDS");
    if (drop_threshold_ && !rank_order_) return fail(MBPE_ERR_ARG, "count_tokens: dropout needs the rank order");
    const uint64_t n_bytes = doc_off[n_docs] - doc_off[0];
    // (special tokens are shorter than their names only as NUL-led markers of the chunk buffer: twice the bytes bounds both)
    if (n_bytes > (~0ull - counts_total_) / repeat / 2)
        return fail(MBPE_ERR_OVERFLOW, "count_tokens: the weighted token total could reach 2^64");
    if (counts_.size() != n_ids) { counts_.assign(n_ids, 0); counts_total_ = 0; }
    std::vector<uint64_t> call(n_ids, 0);
    uint64_t n = 0;
    if (device < 0) {
        for (uint64_t i = 0; i < n_docs; ++i) {
            const std::vector<Token> toks = encode(std::string(text + doc_off[i], doc_off[i + 1] - doc_off[i]), verbose, -1);
            for (Token t : toks)
                if (t < n_ids) call[t] += repeat;      // (an id beyond the table: a NUL-led number in the text itself)
            n += toks.size();
        }
    } else {
        mbpe_encoder *enc = device_encoder(device);
        int rc = mbpe_encoder_counts_reset(enc);
        if (rc == MBPE_OK) rc = mbpe_encoder_set_option(enc, "count_ids", static_cast<int64_t>(n_ids));
        if (rc != MBPE_OK) return rc;
        if (device_split) {
            DeviceSplit ds;
            if ((rc = split_on_device(text, doc_off, n_docs, verbose, device, &ds)) != MBPE_OK) return rc;
            rc = mbpe_encoder_count_endmask(enc, ds.d_text, ds.n_bytes, ds.d_mask, ds.singles.data(), ds.singles.size(),
                                            repeat, &n, nullptr);
        } else {
            std::string buf;
            std::vector<uint64_t> off, first_chunk;
            batch_chunks(text, doc_off, n_docs, verbose, &buf, &off, &first_chunk);
            rc = mbpe_encoder_count(enc, reinterpret_cast<const uint8_t *>(buf.data()), buf.size(), 0, off.data(),
                                    off.size() - 1, repeat, &n, nullptr);
        }
        // the encoder's small table comes back, is added below and is zeroed: a re-created encoder loses nothing
        uint64_t got_ids = 0;
        if (rc == MBPE_OK) rc = mbpe_encoder_counts(enc, call.data(), call.size(), 0, &got_ids, nullptr, nullptr);
        if (rc == MBPE_OK && got_ids != n_ids) rc = fail(MBPE_ERR_STATE, "count_tokens: the encoder's table has another size");
        const int rc_reset = mbpe_encoder_counts_reset(enc);
        if (rc != MBPE_OK) return rc;
        if (rc_reset != MBPE_OK) return rc_reset;
    }
    for (uint64_t i = 0; i < n_ids; ++i) counts_[i] += call[i];
    counts_total_ += repeat * n;
    *n_tokens_out = n;
    if (verbose) std::cout << "Counted " << n_docs << " texts (length " << n_bytes << "): " << n << " tokens\n";
    return MBPE_OK;
}

int Tokenizer::encode_ranges(const char *text, const uint64_t *doc_off, uint64_t n_docs, bool verbose, int device,
                             bool device_split, std::vector<Token> *tokens, std::vector<uint64_t> *ranges,
                             std::vector<uint64_t> *doc_tok_off) {
    tokens->clear();
    ranges->clear();
    doc_tok_off->assign(n_docs + 1, 0);
    if (drop_threshold_ && !rank_order_) {
        set_last_error("encode: dropout needs the rank order (mbpe_tok_set_encode_order)");
        return MBPE_ERR_ARG;
    }
    uint64_t n = 0;
    if (device >= 0 && device_split) {
        // the splitter's text is the original text: tok_byte_off is in the coordinates of the documents' buffer
        DeviceSplit ds;
        int rc = split_on_device(text, doc_off, n_docs, verbose, device, &ds);
        if (rc != MBPE_OK) return rc;
        mbpe_encoder *enc = device_encoder(device);
        tokens->resize(std::max<uint64_t>(ds.n_bytes, 1));
        std::vector<uint64_t> boff(tokens->size() + 1, 0);
        rc = mbpe_encoder_encode_endmask_byteoff(enc, ds.d_text, ds.n_bytes, ds.d_mask, ds.singles.data(),
                                                 ds.singles.size(), ds.doc_off.data(), n_docs, tokens->data(), tokens->size(),
                                                 32, 0, boff.data(), doc_tok_off->data(), &n, nullptr);
        if (rc != MBPE_OK) return rc;
        tokens->resize(n);
        ranges->resize(2 * n);
        for (uint64_t d = 0; d < n_docs; ++d)
            for (uint64_t j = (*doc_tok_off)[d]; j < (*doc_tok_off)[d + 1]; ++j) {
                (*ranges)[2 * j] = boff[j] - ds.doc_off[d];
                (*ranges)[2 * j + 1] = boff[j + 1] - ds.doc_off[d];
            }
        return MBPE_OK;
    }
    // the host split: the encoder reads markers and matches, so every chunk carries its range in its own document
    std::string buf;
    std::vector<uint64_t> off, first_chunk, src, boff;
    batch_chunks(text, doc_off, n_docs, verbose, &buf, &off, &first_chunk, &src);
    const uint64_t n_chunks = off.size() - 1;
    std::vector<uint64_t> chunk_tok(n_chunks + 1, 0);
    if (device >= 0) {
        mbpe_encoder *enc = device_encoder(device);
        tokens->resize(std::max<uint64_t>(buf.size(), 1));
        boff.assign(tokens->size() + 1, 0);
        const int rc = mbpe_encoder_encode_byteoff(enc, reinterpret_cast<const uint8_t *>(buf.data()), buf.size(), 0,
                                                   off.data(), n_chunks, tokens->data(), tokens->size(), 32, 0, boff.data(),
                                                   chunk_tok.data(), &n, nullptr);
        if (rc != MBPE_OK) return rc;
        tokens->resize(n);
    } else {
        // the reference loop; a token covers as many bytes as its vocabulary entry has
        for (uint64_t c = 0; c < n_chunks; ++c) {
            auto vec = text_to_vector(buf.data() + off[c], off[c + 1] - off[c]);
            auto enc = rank_order_ ? encode_rank_ordered(std::move(vec), off[c]) : internal_internal_encode(std::move(vec));
            uint64_t pos = off[c];
            for (Token t : enc) {
                tokens->push_back(t);
                boff.push_back(pos);
                pos += t < vocab_.size() ? vocab_[t].size() : 0;
            }
            chunk_tok[c + 1] = tokens->size();
        }
        boff.push_back(buf.size());
        n = tokens->size();
    }
    // within a chunk the offsets move from the buffer to the chunk's source; its first token starts where the source
    // starts and its last one ends where it ends (a marker's one token is the whole occurrence of the name)
    ranges->resize(2 * n);
    for (uint64_t c = 0; c < n_chunks; ++c) {
        const uint64_t t0 = chunk_tok[c], t1 = chunk_tok[c + 1];
        for (uint64_t j = t0; j < t1; ++j) {
            (*ranges)[2 * j] = j == t0 ? src[2 * c] : src[2 * c] + (boff[j] - off[c]);
            (*ranges)[2 * j + 1] = j + 1 == t1 ? src[2 * c + 1] : src[2 * c] + (boff[j + 1] - off[c]);
        }
    }
    for (uint64_t i = 0; i <= n_docs; ++i) (*doc_tok_off)[i] = chunk_tok[first_chunk[i]];
    if (verbose) std::cout << "Encoded " << n_docs << " texts (length " << buf.size() << ") to " << n << " tokens\n";
    return MBPE_OK;
}

int Tokenizer::encode_batch_packed(const char *text, const uint64_t *doc_off, uint64_t n_docs, bool verbose, int device,
                                   const mbpe_pack_spec *spec, void *ids_out, uint64_t cap_rows, int out_on_device,
                                   uint32_t *len_out, uint64_t *n_rows_out, uint64_t *n_tokens_out,
                                   const mbpe_pack_aux *aux, uint64_t *doc_tok_off_out, bool device_split,
                                   const mbpe_pack_window *win, const struct mbpe_pack_fit *fit) {
    if (device_split) {
        DeviceSplit ds;
        int rc = split_on_device(text, doc_off, n_docs, verbose, device, &ds);
        if (rc != MBPE_OK) return rc;
        mbpe_encoder *enc = device_encoder(device);
        uint64_t n_tokens = 0;
        rc = fit ? mbpe_encoder_encode_batch_endmask_fit(enc, ds.d_text, ds.n_bytes, ds.d_mask, ds.singles.data(),
                                                         ds.singles.size(), ds.doc_off.data(), n_docs, spec, ids_out,
                                                         cap_rows, out_on_device, len_out, n_rows_out, &n_tokens, aux,
                                                         doc_tok_off_out, fit)
           : win ? mbpe_encoder_encode_batch_endmask_windows(enc, ds.d_text, ds.n_bytes, ds.d_mask, ds.singles.data(),
                                                             ds.singles.size(), ds.doc_off.data(), n_docs, spec, ids_out,
                                                             cap_rows, out_on_device, len_out, n_rows_out, &n_tokens, aux,
                                                             doc_tok_off_out, win)
                 : mbpe_encoder_encode_batch_endmask(enc, ds.d_text, ds.n_bytes, ds.d_mask, ds.singles.data(),
                                                     ds.singles.size(), ds.doc_off.data(), n_docs, spec, ids_out, cap_rows,
                                                     out_on_device, len_out, n_rows_out, &n_tokens, aux, doc_tok_off_out);
        if (n_tokens_out) *n_tokens_out = n_tokens;
        if (rc == MBPE_OK && verbose)
            std::cout << "Encoded " << n_docs << " texts (length " << ds.n_bytes << ") to " << n_tokens << " tokens in "
                      << *n_rows_out << " rows\n";
        return rc;
    }
    std::string buf;
    std::vector<uint64_t> off, first_chunk;
    batch_chunks(text, doc_off, n_docs, verbose, &buf, &off, &first_chunk);
    mbpe_encoder *enc = device_encoder(device);
    uint64_t n_tokens = 0;
    const uint8_t *bytes = reinterpret_cast<const uint8_t *>(buf.data());
    const int rc = fit ? mbpe_encoder_encode_batch_fit(enc, bytes, buf.size(), 0, off.data(), off.size() - 1,
                                                       first_chunk.data(), n_docs, spec, ids_out, cap_rows, out_on_device,
                                                       len_out, n_rows_out, &n_tokens, aux, doc_tok_off_out, fit)
                   : win ? mbpe_encoder_encode_batch_windows(enc, bytes, buf.size(), 0, off.data(), off.size() - 1,
                                                           first_chunk.data(), n_docs, spec, ids_out, cap_rows,
                                                           out_on_device, len_out, n_rows_out, &n_tokens, aux,
                                                           doc_tok_off_out, win)
                   : aux ? mbpe_encoder_encode_batch_aux(enc, bytes, buf.size(), 0, off.data(), off.size() - 1,
                                                       first_chunk.data(), n_docs, spec, ids_out, cap_rows, out_on_device,
                                                       len_out, n_rows_out, &n_tokens, aux, doc_tok_off_out)
                       : mbpe_encoder_encode_batch(enc, bytes, buf.size(), 0, off.data(), off.size() - 1,
                                                   first_chunk.data(), n_docs, spec, ids_out, cap_rows, out_on_device,
                                                   len_out, n_rows_out, &n_tokens);
    if (n_tokens_out) *n_tokens_out = n_tokens;
    if (rc == MBPE_OK && verbose)
        std::cout << "Encoded " << n_docs << " texts (length " << buf.size() << ") to " << n_tokens << " tokens in "
                  << *n_rows_out << " rows\n";
    return rc;
}

int Tokenizer::encode_batch_denoise(const char *text, const uint64_t *doc_off, uint64_t n_docs, bool verbose, int device,
                                    const mbpe_denoise_spec *dn, const mbpe_pack_spec *enc_spec,
                                    const mbpe_pack_spec *dec_spec, const mbpe_denoise_batch *out, uint64_t cap_rows,
                                    int out_on_device, uint64_t *n_rows_out, uint64_t *n_tokens_out, bool device_split) {
    uint64_t n_tokens = 0, n_bytes = 0;
    int rc = MBPE_OK;
    if (device_split) {
        DeviceSplit ds;
        rc = split_on_device(text, doc_off, n_docs, verbose, device, &ds);
        if (rc != MBPE_OK) return rc;
        n_bytes = ds.n_bytes;
        rc = mbpe_encoder_encode_batch_endmask_denoise(device_encoder(device), ds.d_text, ds.n_bytes, ds.d_mask,
                                                       ds.singles.data(), ds.singles.size(), ds.doc_off.data(), n_docs, dn,
                                                       enc_spec, dec_spec, out, cap_rows, out_on_device, n_rows_out,
                                                       &n_tokens);
    } else {
        std::string buf;
        std::vector<uint64_t> off, first_chunk;
        batch_chunks(text, doc_off, n_docs, verbose, &buf, &off, &first_chunk);
        n_bytes = buf.size();
        rc = mbpe_encoder_encode_batch_denoise(device_encoder(device), reinterpret_cast<const uint8_t *>(buf.data()),
                                               buf.size(), 0, off.data(), off.size() - 1, first_chunk.data(), n_docs, dn,
                                               enc_spec, dec_spec, out, cap_rows, out_on_device, n_rows_out, &n_tokens);
    }
    if (n_tokens_out) *n_tokens_out = n_tokens;
    if (rc == MBPE_OK && verbose)
        std::cout << "Encoded " << n_docs << " texts (length " << n_bytes << ") to " << n_tokens << " tokens in "
                  << *n_rows_out << " rows of inputs and targets\n";
    return rc;
}

std::vector<std::vector<Token>> Tokenizer::encode_batch(const std::vector<std::string> &texts, bool verbose, int device,
                                                        bool device_split) {
    std::string all;
    std::vector<uint64_t> doc_off{0};
    for (const auto &t : texts) {
        all += t;
        doc_off.push_back(all.size());
    }
    // (a text never makes more tokens than it has bytes: a special token's name, at least one byte, is one token)
    std::vector<Token> flat(all.size());
    std::vector<uint64_t> tok_off;
    uint64_t n = 0;
    const int rc = encode_batch_flat(all.data(), doc_off.data(), texts.size(), verbose, device, flat.data(), flat.size(),
                                     &n, nullptr, &tok_off, device_split);
    if (rc != MBPE_OK) throw mbpe_host::CodedError(rc, mbpe_last_error());
    std::vector<std::vector<Token>> out(texts.size());
    for (size_t i = 0; i < texts.size(); ++i) out[i].assign(flat.begin() + tok_off[i], flat.begin() + tok_off[i + 1]);
    return out;
}

// :725-751
std::string Tokenizer::decode(const std::vector<Token> &tokens, bool verbose, int device) {
    if (verbose) std::cout << "Decoding " << tokens.size() << " tokens\n";
    std::string text;
    if (device >= 0) {
        uint64_t n_invalid = 0;
        const int rc = decode_to_string(device_decoder(device), tokens.data(), tokens.size(), &text, &n_invalid);
        if (rc != MBPE_OK) throw mbpe_host::CodedError(rc, mbpe_last_error());
        if (n_invalid) warn_invalid(tokens.data(), tokens.size());      // rare
        return text;
    }
    for (Token tkn : tokens) {
        auto sp = special_tokens_reverse_lookup_.find(tkn);
        if (sp != special_tokens_reverse_lookup_.end()) { text += sp->second; continue; }
        if (tkn >= vocab_.size()) {
            std::cerr << "Warning: Attempted to decode invalid token ID: " << tkn << "\n";
            continue;
        }
        for (Token c : vocab_[tkn]) text.push_back(static_cast<char>(c));
    }
    return text;
}

int Tokenizer::decode_batch_flat(const Token *tokens, const uint64_t *doc_tok_off, uint64_t n_docs, bool verbose,
                                 int device, uint8_t *bytes_out, uint64_t cap, uint64_t *doc_byte_off_out,
                                 uint64_t *n_out) {
    const uint64_t n = doc_tok_off[n_docs];
    if (verbose) std::cout << "Decoding " << n << " tokens of " << n_docs << " texts\n";
    uint64_t n_invalid = 0;
    const int rc = mbpe_decode_batch(device_decoder(device), tokens, n, 32, 0, doc_tok_off, n_docs, bytes_out, cap, 0,
                                     doc_byte_off_out, n_out, &n_invalid);
    if (n_invalid) warn_invalid(tokens, n);         // (counted whenever the lengths were: also when cap is too small)
    return rc;
}

int Tokenizer::decode_padded(const Token *ids, uint64_t n_rows, uint32_t seq_len, const uint32_t *len, bool verbose,
                             int device, uint8_t *bytes_out, uint64_t cap, uint64_t *doc_byte_off_out, uint64_t *n_out) {
    std::vector<uint64_t> tok_off(n_rows + 1, 0);
    uint64_t n = 0;
    int rc = mbpe_unpack_tokens(device, ids, n_rows, seq_len, 32, 0, len, nullptr, 0, 32, 0, tok_off.data(), &n);
    if (rc != MBPE_OK) return rc;                   // (a length beyond seq_len: before a decoder is created)
    if (verbose) std::cout << "Decoding " << n << " tokens of " << n_rows << " rows\n";
    mbpe_decoder *dec = device_decoder(device);
    void *d_tok = nullptr;
    rc = device_alloc(device, n * sizeof(Token), &d_tok);
    if (rc != MBPE_OK) return rc;
    rc = mbpe_unpack_tokens(device, ids, n_rows, seq_len, 32, 0, len, d_tok, n, 32, 1, nullptr, &n);
    uint64_t n_invalid = 0;
    if (rc == MBPE_OK)
        rc = mbpe_decode_batch(dec, d_tok, n, 32, 1, tok_off.data(), n_rows, bytes_out, cap, 0, doc_byte_off_out, n_out,
                               &n_invalid);
    device_free(d_tok);
    if (n_invalid)
        for (uint64_t r = 0; r < n_rows; ++r) warn_invalid(ids + r * seq_len, len[r]);
    return rc;
}

std::vector<std::string> Tokenizer::decode_batch(const std::vector<std::vector<Token>> &docs, bool verbose, int device) {
    std::vector<Token> flat;
    std::vector<uint64_t> tok_off{0};
    for (const auto &d : docs) {
        flat.insert(flat.end(), d.begin(), d.end());
        tok_off.push_back(flat.size());
    }
    std::vector<uint64_t> byte_off(docs.size() + 1, 0);
    uint64_t n = 0;
    int rc = decode_batch_flat(flat.data(), tok_off.data(), docs.size(), verbose, device, nullptr, 0, byte_off.data(), &n);
    std::string all(n, '\0');
    if (rc == MBPE_OK && n) {
        uint64_t n_invalid = 0;                     // (the query has printed the warnings)
        rc = mbpe_decode_batch(device_decoder(device), flat.data(), flat.size(), 32, 0, tok_off.data(), docs.size(),
                               reinterpret_cast<uint8_t *>(&all[0]), n, 0, byte_off.data(), &n, &n_invalid);
    }
    if (rc != MBPE_OK) throw mbpe_host::CodedError(rc, mbpe_last_error());
    std::vector<std::string> out(docs.size());
    for (size_t i = 0; i < docs.size(); ++i) out[i] = all.substr(byte_off[i], byte_off[i + 1] - byte_off[i]);
    return out;
}

// :754-872
bool Tokenizer::load(const std::string &path, bool verbose) {
    std::ifstream in(path, std::ios::in);
    if (!in.is_open()) {
        std::cerr << "Failed to open file for loading: " << path << "\n";
        return false;
    }
    std::string version;
    std::getline(in, version);
    if (version != "minbpe v1") {
        std::cerr << "Unexpected version: " << version << "\n";
        return false;
    }
    drop_decoder();
    drop_encoder();
    drop_counts();
    drop_splitter();                                            // (the pattern may change)
    merges_lookup_.clear();
    merges_.clear();
    initialize_vocab();
    std::getline(in, pattern_);
    {
        std::string err;   // recompile the pattern of the model file (:770-814)
        if (splitter_.compile(pattern_, &err) != MBPE_OK) {
            std::cerr << "PCRE2 compilation failed on load: " << err << "\n";
            return false;
        }
    }
    int num_special = 0;
    in >> num_special;
    for (int i = 0; i < num_special; i++) {                     // :817-828 (adds to the existing specials)
        std::string token;
        Token id;
        in >> token >> id;
        bool found = false;
        for (auto &kv : special_tokens_)
            if (kv.first == token) { kv.second = id; found = true; }
        if (!found) special_tokens_.emplace_back(token, id);
        special_tokens_reverse_lookup_[id] = token;
        if (verbose) std::cout << "Loaded special token: " << token << " with ID " << id << "\n";
    }
    Token idx1, idx2, cur = 256;
    while (in >> idx1 >> idx2) {                                // :831-837
        merges_.push_back({idx1, idx2});
        merges_lookup_[{idx1, idx2}] = cur++;
    }
    if (verbose) std::cout << "Read input model from \"" << path << "\"\n";
    rebuild_vocab();
    if (verbose)
        std::cout << "Loaded vocab with " << merges_.size() << " merges, vocab size is " << vocab_.size() << "\n";
    return true;
}

// :875-926
bool Tokenizer::save(const std::string &path, bool write_vocab) {
    std::ofstream out(path, std::ios::out);
    if (!out.is_open()) {
        std::cerr << "Unable to open file for saving: " << path << std::endl;
        return false;
    }
    std::cout << "Writing model...\n";
    out << "minbpe v1" << std::endl;
    out << pattern_ << std::endl;
    out << special_tokens_.size() << std::endl;
    for (const auto &st : special_tokens_) out << st.first << ' ' << st.second << std::endl;
    for (const auto &m : merges_) out << m.first << ' ' << m.second << "\n";
    out.close();
    if (write_vocab) {                                          // :894-918
        std::ofstream vf(path + ".vocab", std::ios::out);
        if (!vf.is_open()) {
            std::cerr << "Failed to open .vocab file for writing: " << path + ".vocab" << std::endl;
            return false;
        }
        Token id = 0;
        for (const auto &v : vocab_) {
            vf << std::setw(6) << std::left << id << ": \"";
            for (Token c : v) {
                if (c >= 32 && c <= 126) vf << static_cast<char>(c);
                else vf << "\xEF\xBF\xBD";                      // U+FFFD
            }
            vf << "\"\n";
            id++;
        }
    }
    std::cout << "Complete.\n";
    return true;
}

}  // namespace mbpe_host

// ---- C-ABI (include/mbpe_tokenizer.h) ----------------------------------------

struct mbpe_tokenizer {
    mbpe_host::Tokenizer *t;
};

namespace {
template <typename F>
int guarded(F f) {
    try {
        return f();
    } catch (const std::exception &e) {
        mbpe_host::set_last_error(e.what());
        return MBPE_ERR_ARG;
    }
}
template <typename F>
int coded(F f) {                                     // a CodedError's own code, MBPE_ERR_ARG for anything else
    try {
        f();
        return MBPE_OK;
    } catch (const mbpe_host::CodedError &e) {
        mbpe_host::set_last_error(e.what());
        return e.code;
    } catch (const std::exception &e) {
        mbpe_host::set_last_error(e.what());
        return MBPE_ERR_ARG;
    }
}
int null_argument(const char *who) {
    mbpe_host::set_last_error(std::string(who) + ": NULL argument");
    return MBPE_ERR_ARG;
}
}  // namespace

extern "C" {

int mbpe_tok_create(const char *pattern, mbpe_tokenizer **out) {
    if (!pattern || !out) { mbpe_host::set_last_error("mbpe_tok_create: NULL argument"); return MBPE_ERR_ARG; }
    try {
        *out = new mbpe_tokenizer{new mbpe_host::Tokenizer(pattern)};
        return MBPE_OK;
    } catch (const std::exception &e) {
        mbpe_host::set_last_error(e.what());
        return MBPE_ERR_REGEX;
    }
}

void mbpe_tok_destroy(mbpe_tokenizer *t) {
    if (!t) return;
    delete t->t;
    delete t;
}

int mbpe_tok_set_special_tokens(mbpe_tokenizer *t, const char *text, uint64_t n) {
    if (!t || (!text && n)) return MBPE_ERR_ARG;
    return guarded([&] { t->t->set_special_tokens_from_file(std::string(text ? text : "", n)); return (int)MBPE_OK; });
}

int mbpe_tok_train(mbpe_tokenizer *t, const uint8_t *text, uint64_t n, uint32_t vocab_size, int conflict_resolution,
                   int verbose, int device_id) {
    if (!t || (!text && n)) return MBPE_ERR_ARG;
    return guarded([&] {
        t->t->train(std::string(reinterpret_cast<const char *>(text), n), (int)vocab_size,
                    conflict_resolution ? mbpe_host::Tokenizer::LEXICAL : mbpe_host::Tokenizer::FIRST, verbose != 0,
                    device_id);
        return (int)MBPE_OK;
    });
}

int mbpe_tok_train_split_device(mbpe_tokenizer *t, const uint8_t *text, uint64_t n, uint32_t vocab_size,
                                int conflict_resolution, int verbose, int device_id) {
    if (!t || (!text && n)) return MBPE_ERR_ARG;
    try {
        t->t->train(std::string(reinterpret_cast<const char *>(text), n), (int)vocab_size,
                    conflict_resolution ? mbpe_host::Tokenizer::LEXICAL : mbpe_host::Tokenizer::FIRST, verbose != 0,
                    device_id, true);
        return MBPE_OK;
    } catch (const mbpe_host::CodedError &e) {       // the splitter's own code: MBPE_ERR_ARG for a custom pattern
        mbpe_host::set_last_error(e.what());
        return e.code;
    } catch (const std::exception &e) {
        mbpe_host::set_last_error(e.what());
        return MBPE_ERR_ARG;
    }
}

int mbpe_tok_train_continue(mbpe_tokenizer *t, const uint8_t *text, uint64_t n, uint32_t vocab_size,
                            int conflict_resolution, int verbose, int device_id, int device_split) {
    if (!t || (!text && n)) return MBPE_ERR_ARG;
    try {
        t->t->train(std::string(reinterpret_cast<const char *>(text), n), (int)vocab_size,
                    conflict_resolution ? mbpe_host::Tokenizer::LEXICAL : mbpe_host::Tokenizer::FIRST, verbose != 0,
                    device_id, device_split != 0, true);
        return MBPE_OK;
    } catch (const mbpe_host::CodedError &e) {
        mbpe_host::set_last_error(e.what());
        return e.code;
    } catch (const std::exception &e) {
        mbpe_host::set_last_error(e.what());
        return MBPE_ERR_ARG;
    }
}

int mbpe_tok_train_pieces_begin(mbpe_tokenizer *t, int device_id, int device_split) {
    if (!t) return null_argument("mbpe_tok_train_pieces_begin");
    return coded([&] { t->t->train_pieces_begin(device_id, device_split != 0); });
}

int mbpe_tok_train_pieces_add(mbpe_tokenizer *t, const uint8_t *text, uint64_t n, uint32_t repeat) {
    if (!t || (!text && n)) return null_argument("mbpe_tok_train_pieces_add");
    return coded([&] { t->t->train_pieces_add(reinterpret_cast<const char *>(text), n, repeat); });
}

int mbpe_tok_train_pieces_finish(mbpe_tokenizer *t, uint32_t vocab_size, int conflict_resolution, int verbose, int resume) {
    if (!t) return null_argument("mbpe_tok_train_pieces_finish");
    return coded([&] {
        t->t->train_pieces_finish((int)vocab_size,
                                  conflict_resolution ? mbpe_host::Tokenizer::LEXICAL : mbpe_host::Tokenizer::FIRST,
                                  verbose != 0, resume != 0);
    });
}

int mbpe_tok_train_pieces_export_size(mbpe_tokenizer *t, uint64_t *n_bytes_out) {
    if (!t || !n_bytes_out) return null_argument("mbpe_tok_train_pieces_export_size");
    return coded([&] { *n_bytes_out = t->t->train_pieces_export_size(); });
}

int mbpe_tok_train_pieces_export(mbpe_tokenizer *t, uint8_t *blob_out, uint64_t cap_bytes, uint64_t *n_bytes_out) {
    if (!t || !blob_out) return null_argument("mbpe_tok_train_pieces_export");
    return coded([&] {
        const uint64_t n = t->t->train_pieces_export(blob_out, cap_bytes);
        if (n_bytes_out) *n_bytes_out = n;
    });
}

int mbpe_tok_train_pieces_merge(mbpe_tokenizer *t, const uint8_t *blob, uint64_t n_bytes) {
    if (!t || !blob) return null_argument("mbpe_tok_train_pieces_merge");
    return coded([&] { t->t->train_pieces_merge(blob, n_bytes); });
}

int mbpe_tok_train_pieces_abort(mbpe_tokenizer *t) {
    if (!t) return null_argument("mbpe_tok_train_pieces_abort");
    t->t->train_pieces_abort();
    return MBPE_OK;
}

int mbpe_tok_set_encode_split(mbpe_tokenizer *t, int on_device) {
    if (!t) return MBPE_ERR_ARG;
    t->t->set_encode_split(on_device != 0);
    return MBPE_OK;
}

int mbpe_tok_set_encode_order(mbpe_tokenizer *t, int rank_order) {
    if (!t) return MBPE_ERR_ARG;
    if (rank_order != 0 && rank_order != 1) {
        mbpe_host::set_last_error("mbpe_tok_set_encode_order: rank_order must be 0 or 1");
        return MBPE_ERR_ARG;
    }
    t->t->set_rank_order(rank_order == 1);
    return MBPE_OK;
}

int mbpe_tok_set_encode_dropout(mbpe_tokenizer *t, uint64_t threshold, uint64_t seed) {
    if (!t) return MBPE_ERR_ARG;
    if (threshold > mbpe::kDropoutOne) {
        mbpe_host::set_last_error("mbpe_tok_set_encode_dropout: threshold must not exceed 2^32");
        return MBPE_ERR_ARG;
    }
    t->t->set_dropout(threshold, seed);
    return MBPE_OK;
}

int mbpe_tok_set_encode_fim(mbpe_tokenizer *t, const mbpe_fim_spec *spec) {
    if (!t) return MBPE_ERR_ARG;
    if (spec) {
        const char *msg = "";
        const int rc = mbpe::fim_check_spec(spec, 32, &msg);
        if (rc != MBPE_OK) {
            mbpe_host::set_last_error(std::string("mbpe_tok_set_encode_fim: ") + msg);
            return rc;
        }
    }
    t->t->set_fim(spec);
    return MBPE_OK;
}

int mbpe_tok_set_encode_mlm(mbpe_tokenizer *t, const mbpe_mlm_spec *spec) {
    if (!t) return MBPE_ERR_ARG;
    if (spec) {
        const char *msg = "";
        const int rc = mbpe::mlm_check_spec(spec, 32, &msg);
        if (rc != MBPE_OK) {
            mbpe_host::set_last_error(std::string("mbpe_tok_set_encode_mlm: ") + msg);
            return rc;
        }
    }
    t->t->set_mlm(spec);
    return MBPE_OK;
}

int mbpe_tok_encode_fim_info(mbpe_tokenizer *t, uint8_t *mode_out, uint64_t *cut_out, uint64_t cap_docs,
                             uint64_t *n_docs_out) {
    if (!t || !n_docs_out) {
        mbpe_host::set_last_error("mbpe_tok_encode_fim_info: NULL argument");
        return MBPE_ERR_ARG;
    }
    *n_docs_out = 0;
    mbpe_encoder *enc = t->t->kept_encoder();
    return enc ? mbpe_encoder_fim_info(enc, mode_out, cut_out, cap_docs, n_docs_out) : MBPE_OK;
}

int mbpe_tok_set_train_dedup(mbpe_tokenizer *t, int on) {
    if (!t) return MBPE_ERR_ARG;
    if (on != 0 && on != 1) {
        mbpe_host::set_last_error("mbpe_tok_set_train_dedup: on must be 0 or 1");
        return MBPE_ERR_ARG;
    }
    t->t->set_train_dedup(on == 1);
    return MBPE_OK;
}

int mbpe_tok_set_train_limits(mbpe_tokenizer *t, int64_t min_frequency, int64_t max_token_length) {
    if (!t) return MBPE_ERR_ARG;
    if (min_frequency < 0 || min_frequency > 0x7FFFFFFFll) {
        mbpe_host::set_last_error("mbpe_tok_set_train_limits: min_frequency is 0 (off) .. 2^31 - 1");
        return MBPE_ERR_ARG;
    }
    if (max_token_length != 0 && (max_token_length < 2 || max_token_length > 0x7FFFFFFFll)) {
        mbpe_host::set_last_error("mbpe_tok_set_train_limits: max_token_length is 0 (off), or 2 .. 2^31 - 1 bytes");
        return MBPE_ERR_ARG;
    }
    t->t->set_train_limits(min_frequency, max_token_length);
    return MBPE_OK;
}

int mbpe_tok_set_encode_dedup(mbpe_tokenizer *t, int on) {
    if (!t) return MBPE_ERR_ARG;
    if (on != 0 && on != 1) {
        mbpe_host::set_last_error("mbpe_tok_set_encode_dedup: on must be 0 or 1");
        return MBPE_ERR_ARG;
    }
    t->t->set_encode_dedup(on == 1);
    return MBPE_OK;
}

int mbpe_tok_set_split_unicode(mbpe_tokenizer *t, int on) {
    if (!t) return MBPE_ERR_ARG;
    t->t->set_split_unicode(on != 0);
    return MBPE_OK;
}

int mbpe_tok_set_merges(mbpe_tokenizer *t, const uint32_t *merges, uint32_t n_merges) {
    if (!t || (!merges && n_merges)) return MBPE_ERR_ARG;
    std::vector<mbpe_host::TokenPair> m;
    for (uint32_t k = 0; k < n_merges; ++k) m.push_back({merges[2 * k], merges[2 * k + 1]});
    t->t->set_merges(m);
    return MBPE_OK;
}

int mbpe_tok_get_merges(mbpe_tokenizer *t, uint32_t *merges_out, uint32_t cap, uint32_t *n_out) {
    if (!t || !n_out) return MBPE_ERR_ARG;
    const auto &m = t->t->get_merges();
    *n_out = (uint32_t)m.size();
    if (!merges_out) return MBPE_OK;
    if (cap < m.size()) { mbpe_host::set_last_error("merges_out too small"); return MBPE_ERR_ARG; }
    for (size_t k = 0; k < m.size(); ++k) { merges_out[2 * k] = m[k].first; merges_out[2 * k + 1] = m[k].second; }
    return MBPE_OK;
}

int mbpe_tok_save(mbpe_tokenizer *t, const char *path, int write_vocab) {
    if (!t || !path) return MBPE_ERR_ARG;
    return guarded([&] { return t->t->save(path, write_vocab != 0) ? (int)MBPE_OK : (int)MBPE_ERR_IO; });
}

int mbpe_tok_load(mbpe_tokenizer *t, const char *path, int verbose) {
    if (!t || !path) return MBPE_ERR_ARG;
    return guarded([&] { return t->t->load(path, verbose != 0) ? (int)MBPE_OK : (int)MBPE_ERR_IO; });
}

int mbpe_tok_encode(mbpe_tokenizer *t, const uint8_t *text, uint64_t n, int verbose, uint32_t *tokens_out,
                    uint64_t cap, uint64_t *n_out) {
    if (!t || (!text && n) || !n_out) return MBPE_ERR_ARG;
    return guarded([&] {
        auto enc = t->t->encode(std::string(reinterpret_cast<const char *>(text), n), verbose != 0);
        *n_out = enc.size();
        if (!tokens_out) return (int)MBPE_OK;
        if (cap < enc.size()) { mbpe_host::set_last_error("tokens_out too small"); return (int)MBPE_ERR_ARG; }
        memcpy(tokens_out, enc.data(), enc.size() * sizeof(uint32_t));
        return (int)MBPE_OK;
    });
}

int mbpe_tok_encode_device(mbpe_tokenizer *t, const uint8_t *text, uint64_t n, int verbose, int device_id,
                           uint32_t *tokens_out, uint64_t cap, uint64_t *n_out) {
    if (!t || (!text && n) || !n_out || device_id < 0) return MBPE_ERR_ARG;
    try {
        auto enc = t->t->encode(std::string(reinterpret_cast<const char *>(text), n), verbose != 0, device_id,
                                t->t->encode_split());
        *n_out = enc.size();
        if (!tokens_out) return MBPE_OK;
        if (cap < enc.size()) { mbpe_host::set_last_error("tokens_out too small"); return MBPE_ERR_ARG; }
        memcpy(tokens_out, enc.data(), enc.size() * sizeof(uint32_t));
        return MBPE_OK;
    } catch (const mbpe_host::CodedError &e) {      // mbpe_encode_chunks failed: its own code (no device, memory, HIP, ids)
        mbpe_host::set_last_error(e.what());
        return e.code;
    } catch (const std::exception &e) {
        mbpe_host::set_last_error(e.what());
        return MBPE_ERR_ARG;
    }
}

int mbpe_tok_encode_batch_device(mbpe_tokenizer *t, const uint8_t *text, const uint64_t *doc_off, uint64_t n_docs,
                                 int verbose, int device_id, uint32_t *tokens_out, uint64_t cap,
                                 uint64_t *doc_tok_off_out, uint64_t *n_out) {
    if (n_out) *n_out = 0;
    if (!t || !n_out || !doc_off || device_id < 0 || (!text && doc_off[n_docs] > doc_off[0])) {
        mbpe_host::set_last_error("mbpe_tok_encode_batch_device: NULL argument or negative device");
        return MBPE_ERR_ARG;
    }
    for (uint64_t i = 0; i < n_docs; ++i)
        if (doc_off[i + 1] < doc_off[i]) { mbpe_host::set_last_error("doc_off must be ascending"); return MBPE_ERR_ARG; }
    try {
        // tokens_out, cap and n_out go to the encoder as they are: a query copies no token, a cap too small writes none
        std::vector<uint64_t> tok_off;
        const int rc = t->t->encode_batch_flat(reinterpret_cast<const char *>(text), doc_off, n_docs, verbose != 0,
                                               device_id, tokens_out, cap, n_out, nullptr, &tok_off,
                                               t->t->encode_split());
        if (rc != MBPE_OK) return rc;
        if (doc_tok_off_out) memcpy(doc_tok_off_out, tok_off.data(), tok_off.size() * sizeof(uint64_t));
        return MBPE_OK;
    } catch (const mbpe_host::CodedError &e) {      // mbpe_encoder_create failed: its own code
        mbpe_host::set_last_error(e.what());
        return e.code;
    } catch (const std::exception &e) {
        mbpe_host::set_last_error(e.what());
        return MBPE_ERR_ARG;
    }
}

int mbpe_tok_count_tokens(mbpe_tokenizer *t, const uint8_t *text, const uint64_t *doc_off, uint64_t n_docs, int verbose,
                          int device_id, uint64_t repeat, uint64_t *n_tokens_out) {
    if (n_tokens_out) *n_tokens_out = 0;
    if (!t || !n_tokens_out || !doc_off || (!text && doc_off[n_docs] > doc_off[0])) return null_argument("mbpe_tok_count_tokens");
    for (uint64_t i = 0; i < n_docs; ++i)
        if (doc_off[i + 1] < doc_off[i]) { mbpe_host::set_last_error("doc_off must be ascending"); return MBPE_ERR_ARG; }
    try {
        return t->t->count_tokens(reinterpret_cast<const char *>(text), doc_off, n_docs, verbose != 0, device_id, repeat,
                                  n_tokens_out, t->t->encode_split());
    } catch (const mbpe_host::CodedError &e) {
        mbpe_host::set_last_error(e.what());
        return e.code;
    } catch (const std::exception &e) {
        mbpe_host::set_last_error(e.what());
        return MBPE_ERR_ARG;
    }
}

int mbpe_tok_token_counts(mbpe_tokenizer *t, uint64_t *counts_out, uint64_t cap_ids, uint64_t *n_ids_out,
                          uint64_t *n_tokens_out) {
    if (!t) return null_argument("mbpe_tok_token_counts");
    const std::vector<uint64_t> &c = t->t->token_counts();
    const uint64_t n_ids = c.empty() ? t->t->count_ids() : c.size();
    if (n_ids_out) *n_ids_out = n_ids;
    if (n_tokens_out) *n_tokens_out = t->t->token_counts_total();
    if (!counts_out) return MBPE_OK;
    if (cap_ids < n_ids) { mbpe_host::set_last_error("counts_out too small"); return MBPE_ERR_ARG; }
    if (c.empty()) memset(counts_out, 0, n_ids * sizeof(uint64_t));
    else memcpy(counts_out, c.data(), n_ids * sizeof(uint64_t));
    return MBPE_OK;
}

int mbpe_tok_token_counts_reset(mbpe_tokenizer *t) {
    if (!t) return null_argument("mbpe_tok_token_counts_reset");
    t->t->drop_counts();
    return MBPE_OK;
}

// the two _byteoff calls after their checks: one encode_ranges, then what the caller has room for
static int tok_encode_ranges(mbpe_tokenizer *t, const uint8_t *text, const uint64_t *doc_off, uint64_t n_docs, int verbose,
                             int device_id, uint32_t *tokens_out, uint64_t *ranges_out, uint64_t cap,
                             uint64_t *doc_tok_off_out, uint64_t *n_out) {
    try {
        std::vector<mbpe_host::Token> tokens;
        std::vector<uint64_t> ranges, tok_off;
        const int rc = t->t->encode_ranges(reinterpret_cast<const char *>(text), doc_off, n_docs, verbose != 0, device_id,
                                           device_id >= 0 && t->t->encode_split(), &tokens, &ranges, &tok_off);
        if (rc != MBPE_OK) return rc;
        *n_out = tokens.size();
        if (doc_tok_off_out) doc_tok_off_out[0] = 0;
        if (tokens_out && cap < tokens.size()) { mbpe_host::set_last_error("tokens_out too small"); return MBPE_ERR_ARG; }
        if (doc_tok_off_out) memcpy(doc_tok_off_out, tok_off.data(), tok_off.size() * sizeof(uint64_t));
        if (!tokens_out) return MBPE_OK;
        if (!tokens.empty()) {
            memcpy(tokens_out, tokens.data(), tokens.size() * sizeof(uint32_t));
            memcpy(ranges_out, ranges.data(), ranges.size() * sizeof(uint64_t));
        }
        return MBPE_OK;
    } catch (const mbpe_host::CodedError &e) {      // the encoder's or the splitter's own code
        mbpe_host::set_last_error(e.what());
        return e.code;
    } catch (const std::exception &e) {
        mbpe_host::set_last_error(e.what());
        return MBPE_ERR_ARG;
    }
}

int mbpe_tok_encode_byteoff(mbpe_tokenizer *t, const uint8_t *text, uint64_t n, int verbose, int device_id,
                            uint32_t *tokens_out, uint64_t *ranges_out, uint64_t cap, uint64_t *n_out) {
    if (n_out) *n_out = 0;
    if (!t || !n_out || (!text && n) || (tokens_out && !ranges_out)) {
        mbpe_host::set_last_error("mbpe_tok_encode_byteoff: NULL argument");
        return MBPE_ERR_ARG;
    }
    const uint64_t doc_off[2] = {0, n};
    return tok_encode_ranges(t, text, doc_off, 1, verbose, device_id, tokens_out, ranges_out, cap, nullptr, n_out);
}

int mbpe_tok_encode_batch_byteoff_device(mbpe_tokenizer *t, const uint8_t *text, const uint64_t *doc_off, uint64_t n_docs,
                                         int verbose, int device_id, uint32_t *tokens_out, uint64_t *ranges_out,
                                         uint64_t cap, uint64_t *doc_tok_off_out, uint64_t *n_out) {
    if (n_out) *n_out = 0;
    if (!t || !n_out || !doc_off || device_id < 0 || (!text && doc_off[n_docs] > doc_off[0]) ||
        (tokens_out && !ranges_out)) {
        mbpe_host::set_last_error("mbpe_tok_encode_batch_byteoff_device: NULL argument or negative device");
        return MBPE_ERR_ARG;
    }
    for (uint64_t i = 0; i < n_docs; ++i)
        if (doc_off[i + 1] < doc_off[i]) { mbpe_host::set_last_error("doc_off must be ascending"); return MBPE_ERR_ARG; }
    return tok_encode_ranges(t, text, doc_off, n_docs, verbose, device_id, tokens_out, ranges_out, cap, doc_tok_off_out,
                             n_out);
}

int mbpe_tok_encode_batch_packed_device(mbpe_tokenizer *t, const uint8_t *text, const uint64_t *doc_off, uint64_t n_docs,
                                        int verbose, int device_id, const mbpe_pack_spec *spec, void *ids_out,
                                        uint64_t cap_rows, int out_on_device, uint32_t *len_out, uint64_t *n_rows_out,
                                        uint64_t *n_tokens_out) {
    if (n_rows_out) *n_rows_out = 0;
    if (n_tokens_out) *n_tokens_out = 0;
    if (!t || !n_rows_out || !doc_off || !spec || device_id < 0 || (!text && doc_off[n_docs] > doc_off[0])) {
        mbpe_host::set_last_error("mbpe_tok_encode_batch_packed_device: NULL argument or negative device");
        return MBPE_ERR_ARG;
    }
    for (uint64_t i = 0; i < n_docs; ++i)
        if (doc_off[i + 1] < doc_off[i]) { mbpe_host::set_last_error("doc_off must be ascending"); return MBPE_ERR_ARG; }
    try {
        return t->t->encode_batch_packed(reinterpret_cast<const char *>(text), doc_off, n_docs, verbose != 0, device_id,
                                         spec, ids_out, cap_rows, out_on_device, len_out, n_rows_out, n_tokens_out,
                                         nullptr, nullptr, t->t->encode_split());
    } catch (const mbpe_host::CodedError &e) {      // mbpe_encoder_create failed: its own code
        mbpe_host::set_last_error(e.what());
        return e.code;
    } catch (const std::exception &e) {
        mbpe_host::set_last_error(e.what());
        return MBPE_ERR_ARG;
    }
}

int mbpe_tok_encode_batch_aux_device(mbpe_tokenizer *t, const uint8_t *text, const uint64_t *doc_off, uint64_t n_docs,
                                     int verbose, int device_id, const mbpe_pack_spec *spec, void *ids_out,
                                     uint64_t cap_rows, int out_on_device, uint32_t *len_out, uint64_t *n_rows_out,
                                     uint64_t *n_tokens_out, const mbpe_pack_aux *aux, uint64_t *doc_tok_off_out) {
    if (n_rows_out) *n_rows_out = 0;
    if (n_tokens_out) *n_tokens_out = 0;
    if (!t || !n_rows_out || !doc_off || !spec || !aux || device_id < 0 || (!text && doc_off[n_docs] > doc_off[0])) {
        mbpe_host::set_last_error("mbpe_tok_encode_batch_aux_device: NULL argument or negative device");
        return MBPE_ERR_ARG;
    }
    for (uint64_t i = 0; i < n_docs; ++i)
        if (doc_off[i + 1] < doc_off[i]) { mbpe_host::set_last_error("doc_off must be ascending"); return MBPE_ERR_ARG; }
    try {
        return t->t->encode_batch_packed(reinterpret_cast<const char *>(text), doc_off, n_docs, verbose != 0, device_id,
                                         spec, ids_out, cap_rows, out_on_device, len_out, n_rows_out, n_tokens_out, aux,
                                         doc_tok_off_out, t->t->encode_split());
    } catch (const mbpe_host::CodedError &e) {      // mbpe_encoder_create failed: its own code
        mbpe_host::set_last_error(e.what());
        return e.code;
    } catch (const std::exception &e) {
        mbpe_host::set_last_error(e.what());
        return MBPE_ERR_ARG;
    }
}

int mbpe_tok_encode_batch_denoise_device(mbpe_tokenizer *t, const uint8_t *text, const uint64_t *doc_off, uint64_t n_docs,
                                         int verbose, int device_id, const mbpe_denoise_spec *dn,
                                         const mbpe_pack_spec *enc_spec, const mbpe_pack_spec *dec_spec,
                                         const mbpe_denoise_batch *out, uint64_t cap_rows, int out_on_device,
                                         uint64_t *n_rows_out, uint64_t *n_tokens_out) {
    if (n_rows_out) *n_rows_out = 0;
    if (n_tokens_out) *n_tokens_out = 0;
    if (!t || !n_rows_out || !doc_off || !dn || !enc_spec || !dec_spec || !out || device_id < 0 ||
        (!text && doc_off[n_docs] > doc_off[0])) {
        mbpe_host::set_last_error("mbpe_tok_encode_batch_denoise_device: NULL argument or negative device");
        return MBPE_ERR_ARG;
    }
    for (uint64_t i = 0; i < n_docs; ++i)
        if (doc_off[i + 1] < doc_off[i]) { mbpe_host::set_last_error("doc_off must be ascending"); return MBPE_ERR_ARG; }
    try {
        return t->t->encode_batch_denoise(reinterpret_cast<const char *>(text), doc_off, n_docs, verbose != 0, device_id, dn,
                                          enc_spec, dec_spec, out, cap_rows, out_on_device, n_rows_out, n_tokens_out,
                                          t->t->encode_split());
    } catch (const mbpe_host::CodedError &e) {      // mbpe_encoder_create failed: its own code
        mbpe_host::set_last_error(e.what());
        return e.code;
    } catch (const std::exception &e) {
        mbpe_host::set_last_error(e.what());
        return MBPE_ERR_ARG;
    }
}

int mbpe_tok_encode_batch_windows_device(mbpe_tokenizer *t, const uint8_t *text, const uint64_t *doc_off, uint64_t n_docs,
                                         int verbose, int device_id, const mbpe_pack_spec *spec, void *ids_out,
                                         uint64_t cap_rows, int out_on_device, uint32_t *len_out, uint64_t *n_rows_out,
                                         uint64_t *n_tokens_out, const mbpe_pack_aux *aux, uint64_t *doc_tok_off_out,
                                         const mbpe_pack_window *win) {
    if (n_rows_out) *n_rows_out = 0;
    if (n_tokens_out) *n_tokens_out = 0;
    if (!t || !n_rows_out || !doc_off || !spec || !aux || !win || device_id < 0 ||
        (!text && doc_off[n_docs] > doc_off[0])) {
        mbpe_host::set_last_error("mbpe_tok_encode_batch_windows_device: NULL argument or negative device");
        return MBPE_ERR_ARG;
    }
    for (uint64_t i = 0; i < n_docs; ++i)
        if (doc_off[i + 1] < doc_off[i]) { mbpe_host::set_last_error("doc_off must be ascending"); return MBPE_ERR_ARG; }
    try {
        return t->t->encode_batch_packed(reinterpret_cast<const char *>(text), doc_off, n_docs, verbose != 0, device_id,
                                         spec, ids_out, cap_rows, out_on_device, len_out, n_rows_out, n_tokens_out, aux,
                                         doc_tok_off_out, t->t->encode_split(), win);
    } catch (const mbpe_host::CodedError &e) {      // mbpe_encoder_create failed: its own code
        mbpe_host::set_last_error(e.what());
        return e.code;
    } catch (const std::exception &e) {
        mbpe_host::set_last_error(e.what());
        return MBPE_ERR_ARG;
    }
}

int mbpe_tok_encode_batch_fit_device(mbpe_tokenizer *t, const uint8_t *text, const uint64_t *doc_off, uint64_t n_docs,
                                     int verbose, int device_id, const mbpe_pack_spec *spec, void *ids_out,
                                     uint64_t cap_rows, int out_on_device, uint32_t *len_out, uint64_t *n_rows_out,
                                     uint64_t *n_tokens_out, const mbpe_pack_aux *aux, uint64_t *doc_tok_off_out,
                                     const struct mbpe_pack_fit *fit) {
    if (n_rows_out) *n_rows_out = 0;
    if (n_tokens_out) *n_tokens_out = 0;
    if (!t || !n_rows_out || !doc_off || !spec || !aux || !fit || device_id < 0 ||
        (!text && doc_off[n_docs] > doc_off[0])) {
        mbpe_host::set_last_error("mbpe_tok_encode_batch_fit_device: NULL argument or negative device");
        return MBPE_ERR_ARG;
    }
    for (uint64_t i = 0; i < n_docs; ++i)
        if (doc_off[i + 1] < doc_off[i]) { mbpe_host::set_last_error("doc_off must be ascending"); return MBPE_ERR_ARG; }
    try {
        return t->t->encode_batch_packed(reinterpret_cast<const char *>(text), doc_off, n_docs, verbose != 0, device_id,
                                         spec, ids_out, cap_rows, out_on_device, len_out, n_rows_out, n_tokens_out, aux,
                                         doc_tok_off_out, t->t->encode_split(), nullptr, fit);
    } catch (const mbpe_host::CodedError &e) {      // mbpe_encoder_create failed: its own code
        mbpe_host::set_last_error(e.what());
        return e.code;
    } catch (const std::exception &e) {
        mbpe_host::set_last_error(e.what());
        return MBPE_ERR_ARG;
    }
}

int mbpe_tok_decode_padded_device(mbpe_tokenizer *t, const uint32_t *ids, uint64_t n_rows, uint32_t seq_len,
                                  const uint32_t *len, int verbose, int device_id, uint8_t *bytes_out, uint64_t cap,
                                  uint64_t *doc_byte_off_out, uint64_t *n_out) {
    if (n_out) *n_out = 0;
    if (!t || !n_out || !doc_byte_off_out || device_id < 0 || ((!ids || !len) && n_rows)) {
        mbpe_host::set_last_error("mbpe_tok_decode_padded_device: NULL argument or negative device");
        return MBPE_ERR_ARG;
    }
    try {
        return t->t->decode_padded(ids, n_rows, seq_len, len, verbose != 0, device_id, bytes_out, cap, doc_byte_off_out,
                                   n_out);
    } catch (const mbpe_host::CodedError &e) {      // mbpe_decoder_create failed: its own code
        mbpe_host::set_last_error(e.what());
        return e.code;
    } catch (const std::exception &e) {
        mbpe_host::set_last_error(e.what());
        return MBPE_ERR_ARG;
    }
}

int mbpe_tok_decode_device(mbpe_tokenizer *t, const uint32_t *tokens, uint64_t n, int verbose, int device_id,
                           uint8_t *bytes_out, uint64_t cap, uint64_t *n_out) {
    if (!t || (!tokens && n) || !n_out || device_id < 0) return MBPE_ERR_ARG;
    try {
        auto s = t->t->decode(std::vector<mbpe_host::Token>(tokens, tokens + n), verbose != 0, device_id);
        *n_out = s.size();
        if (!bytes_out) return MBPE_OK;
        if (cap < s.size()) { mbpe_host::set_last_error("bytes_out too small"); return MBPE_ERR_ARG; }
        memcpy(bytes_out, s.data(), s.size());
        return MBPE_OK;
    } catch (const mbpe_host::CodedError &e) {      // mbpe_decoder_create / mbpe_decode_tokens failed: its own code
        mbpe_host::set_last_error(e.what());
        return e.code;
    } catch (const std::exception &e) {
        mbpe_host::set_last_error(e.what());
        return MBPE_ERR_ARG;
    }
}

int mbpe_tok_decode_batch_device(mbpe_tokenizer *t, const uint32_t *tokens, const uint64_t *doc_tok_off,
                                 uint64_t n_docs, int verbose, int device_id, uint8_t *bytes_out, uint64_t cap,
                                 uint64_t *doc_byte_off_out, uint64_t *n_out) {
    if (n_out) *n_out = 0;
    if (!t || !n_out || !doc_tok_off || !doc_byte_off_out || device_id < 0 || (!tokens && doc_tok_off[n_docs])) {
        mbpe_host::set_last_error("mbpe_tok_decode_batch_device: NULL argument or negative device");
        return MBPE_ERR_ARG;
    }
    const int rc = mbpe_host::check_doc_tok_off(doc_tok_off, n_docs, doc_tok_off[n_docs]);
    if (rc != MBPE_OK) return rc;
    try {
        return t->t->decode_batch_flat(tokens, doc_tok_off, n_docs, verbose != 0, device_id, bytes_out, cap,
                                       doc_byte_off_out, n_out);
    } catch (const mbpe_host::CodedError &e) {      // mbpe_decoder_create failed: its own code
        mbpe_host::set_last_error(e.what());
        return e.code;
    } catch (const std::exception &e) {
        mbpe_host::set_last_error(e.what());
        return MBPE_ERR_ARG;
    }
}

int mbpe_tok_decode(mbpe_tokenizer *t, const uint32_t *tokens, uint64_t n, int verbose, uint8_t *bytes_out,
                    uint64_t cap, uint64_t *n_out) {
    if (!t || (!tokens && n) || !n_out) return MBPE_ERR_ARG;
    return guarded([&] {
        auto s = t->t->decode(std::vector<mbpe_host::Token>(tokens, tokens + n), verbose != 0);
        *n_out = s.size();
        if (!bytes_out) return (int)MBPE_OK;
        if (cap < s.size()) { mbpe_host::set_last_error("bytes_out too small"); return (int)MBPE_ERR_ARG; }
        memcpy(bytes_out, s.data(), s.size());
        return (int)MBPE_OK;
    });
}

}  // extern "C"
