// Host-side C++ layer above the C-ABI (include/mbpe.h): the pieces of the
// reference's Tokenizer that surround the hot path -- regex pre-split, the
// "minbpe v1" model file, encode / decode -- mirrored with the reference's
// names and argument meaning so that callers and tests read like the
// reference's own (code/include/Tokenizer.h:379-927).
#ifndef MBPE_HOST_H
#define MBPE_HOST_H

#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

struct mbpe_ctx;
struct mbpe_decoder;
struct mbpe_encoder;

namespace mbpe_host {

// last error text of the calling thread (returned by mbpe_last_error())
void set_last_error(const std::string &msg);
const char *last_error();

// a failed C-ABI call inside the C++ layer: the MBPE_ERR_* code travels with the text
struct CodedError : std::runtime_error {
    int code;
    CodedError(int c, const std::string &msg) : std::runtime_error(msg), code(c) {}
};

// HIP device of a training context (csrc/train.cpp)
int ctx_device(const mbpe_ctx *c);

// mbpe_decode_tokens (csrc/decode.hip) for host tokens into a string that is sized between the length pass and the
// copy, so that the tokens are uploaded once; returns an mbpe_status
int decode_to_string(mbpe_decoder *d, const uint32_t *tokens, uint64_t n, std::string *out, uint64_t *n_invalid);

// the doc_tok_off rule of mbpe_decode_batch (csrc/decode.hip): n_docs + 1 ascending offsets from 0 to n_tokens;
// MBPE_OK, or MBPE_ERR_ARG with the last error set.  Touches no device
int check_doc_tok_off(const uint64_t *doc_tok_off, uint64_t n_docs, uint64_t n_tokens);

// device memory of HIP device `device` for host code that only hands it on (csrc/pack.hip); an mbpe_status
int device_alloc(int device, uint64_t n_bytes, void **out);
void device_free(void *p);

// Tokenizer.h:59-60; nullptr for an unknown encoder name
const char *split_pattern_for(const std::string &encoder);

// host threads for PCRE2 work on n_bytes of text: MBPE_SPLIT_THREADS (environment; default 16), capped by the
// hardware's threads and by one thread per MiB; at least 1
unsigned split_thread_count(uint64_t n_bytes);

// What PCRE2 says of every Unicode scalar value under the options of Splitter::compile, for the device split's
// "unicode" mode (csrc/split_rule.h): cls = 2 bits per value (bits 2 (cp & 15) .. of word cp >> 4: 0 = \p{L}, 1 = \p{N},
// 2 = \s, 3 = none of them; the surrogates read 3), fold = the values >= 0x80 that match one of s d m t l v e r under
// PCRE2_CASELESS, each with that letter.  Asked of the library once per process, on the first call; nullptr with *err
// set when the library is missing, disagrees with split_class below 0x80, or folds more than 8 values.
struct SplitUnicodeTable {
    std::vector<uint32_t> cls;
    uint32_t n_fold = 0;
    uint32_t fold_cp[8] = {0};
    uint8_t fold_to[8] = {0};
    double build_ms = 0.0;
};
const SplitUnicodeTable *split_unicode_table(std::string *err);

// Compiled split pattern + match loop (Tokenizer.h:391-451, :506-540).
class Splitter {
public:
    Splitter() = default;
    ~Splitter();
    Splitter(const Splitter &) = delete;
    Splitter &operator=(const Splitter &) = delete;

    int compile(const std::string &pattern, std::string *err);   // replaces any earlier pattern
    void reset();
    // chunk c = [starts[c], ends[c]); empty pattern -> one chunk = whole text
    int split(const uint8_t *text, uint64_t n, std::vector<uint64_t> *starts,
              std::vector<uint64_t> *ends, std::string *err) const;
    // The match loop over n_spans stretches [spans[2 k], spans[2 k + 1]) (ascending, disjoint) of a text of n bytes,
    // each matched from its start on its own subject [a, min(b + 1, n)) by up to n_threads threads; `sub` holds the
    // text from byte `origin` on.  last_bytes receives, ascending, the last byte of every match.  MBPE_ERR_SPLIT_GAP
    // when the matches of a stretch do not tile it.  end_is_cut (optional, one flag per stretch): the stretch ends
    // where another text begins (mbpe_splitter_split_docs) and its subject is [a, b).
    // (csrc/split.hip: the host spans of the device split)
    int split_spans(const uint8_t *sub, uint64_t origin, uint64_t n, const uint64_t *spans, uint64_t n_spans,
                    unsigned n_threads, std::vector<uint64_t> *last_bytes, std::string *err,
                    const uint8_t *end_is_cut = nullptr) const;
    bool has_pattern() const { return code_ != nullptr; }
    const std::string &pattern() const { return pattern_; }

private:
    std::string pattern_;
    void *code_ = nullptr;
    void *match_data_ = nullptr;
};

}  // namespace mbpe_host

#endif
