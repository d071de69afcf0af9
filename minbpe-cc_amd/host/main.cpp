// minbpe-cc: the reference's command line (code/examples/minbpe-cc.cpp:92-265)
// on top of the MI355X training path.  Same flags, defaults, messages and exit
// codes; `--train -c lexical` runs on the GPU.  The only additions are --device, the --device-* switches, --rank-order,
// --dropout / --seed, --byte-ranges-out, --continue-from, --input-list, --count / --counts / --counts-out, and
// --token-counts-out.
#include "mbpe.h"
#include "mbpe_tokenizer.h"

#include <chrono>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <sys/stat.h>
#include <vector>

using Token = uint32_t;   // Tokenizer.h:38

namespace {

bool exists(const std::string &p) {
    struct stat st;
    return stat(p.c_str(), &st) == 0;
}

bool load_file_to_string(const std::string &path, std::string *out, std::string *err) {   // :36-46
    std::ifstream file(path);
    if (!file) { *err = std::strerror(errno); return false; }
    std::stringstream buffer;
    buffer << file.rdbuf();
    *out = buffer.str();
    return true;
}

bool save_encoding(const std::string &path, const std::vector<Token> &encoded, std::string *err) {   // :58-69
    std::ofstream file(path, std::ios::binary);
    if (!file) { *err = std::strerror(errno); return false; }
    for (const auto &code : encoded) file.write(reinterpret_cast<const char *>(&code), sizeof(Token));
    return true;
}

bool load_encoding(const std::string &path, std::vector<Token> *data, std::string *err) {   // :71-89
    std::ifstream file(path, std::ios::binary);
    if (!file.is_open()) { *err = std::strerror(errno); return false; }
    Token number;
    while (file.read(reinterpret_cast<char *>(&number), sizeof(Token))) data->push_back(number);
    std::cout << "Loaded encoding with " << data->size() << " tokens\n";
    return true;
}

void usage() {
    std::cout << "Training, encoding and decoding of tokens\nUsage: minbpe-cc [OPTIONS]\n\nOptions:\n"
                 "  -h,--help                   Print this help message and exit\n"
                 "  -i,--input TEXT             Path to the input to be trained on, encoded or decoded\n"
                 "  -o,--output TEXT            Path for the output of the encoding or decoding\n"
                 "  -s,--special-tokens-path TEXT\n                              Path to the special tokens file\n"
                 "  -t,--train                  Train on the input\n"
                 "  -d,--decode                 Decode the input\n"
                 "  -e,--encode                 Encode the input\n"
                 "  -w,--write-vocab            When training, write the vocabulary to a file\n"
                 "  --vocab-size INT            Vocabulary size\n"
                 "  --encoder TEXT              Encoder to use from basic,gpt2,gpt4\n"
                 "  -m,--model-path TEXT        Path to load or save the model\n"
                 "  -v,--verbose                Print more things\n"
                 "  -c,--conflict-resolution TEXT:{first,lexical}\n"
                 "                              Conflict resolution strategy: 'first' or 'lexical'\n"
                 "  --device INT                HIP device used for training (default 0)\n"
                 "  --device-encode             When encoding, apply the merges on the HIP device (--device)\n"
                 "  --device-decode             When decoding, expand the tokens on the HIP device (--device)\n"
                 "  --device-split              When training with gpt2 or gpt4, split the text on the HIP device (--device);\n"
                 "                              when encoding, only together with --device-encode: the text is cut at the\n"
                 "                              special tokens and split on the device too (without it: no effect)\n"
                 "  --device-split-unicode      --device-split, with non-ASCII text split on the device as well\n"
                 "  --rank-order                When encoding, apply the merges in rank order (a chunk's pair with the lowest\n"
                 "                              merge id first: the segmentation the model was trained on) instead of the\n"
                 "                              reference's greedy passes; on the host and with --device-encode\n"
                 "  --dropout FLOAT             When encoding with --rank-order: BPE-dropout, a merge that applies is skipped with\n"
                 "                              this probability (0 .. 1), so the text gets another segmentation per --seed;\n"
                 "                              on the host, with --device-encode and with --device-split.  Without\n"
                 "                              --rank-order it is a usage error\n"
                 "  --seed UINT                 The seed of --dropout (default 0); the same seed gives the same tokens\n"
                 "  --byte-ranges-out TEXT      When encoding, also write one line \"start end\" per token to this file: the bytes\n"
                 "                              of the input the token stands for (a special token: its name's occurrence);\n"
                 "                              on the host, with --device-encode, --device-split and --rank-order alike\n"
                 "  --dedup                     With --train: split as asked, then train on the distinct chunks with their counts\n"
                 "                              (deduplicated on the HIP device): the same model.  One pass over the unique\n"
                 "                              chunks per merge: meant for -c first, for vocabularies beyond 65,536 and for\n"
                 "                              --continue-from; -c lexical below that is faster without it, and --encoder\n"
                 "                              basic has one chunk, so nothing is saved.  Combines with --device-split,\n"
                 "                              --device-split-unicode, --continue-from and --conflict-resolution.\n"
                 "                              With --encode --device-encode: deduplicate the chunks on the device, encode\n"
                 "                              the distinct ones and copy their tokens to every occurrence: the same output,\n"
                 "                              with or without --device-split, --device-split-unicode and --rank-order;\n"
                 "                              meant for large texts of natural language in rank order.  With --dropout or\n"
                 "                              --byte-ranges-out it is an error; without --device-encode it has no effect\n"
                 "  --continue-from TEXT        With --train: load this model and continue its training on the input up to\n"
                 "                              --vocab-size, which must not be below the model's size; the result goes to\n"
                 "                              --model-path.  The loaded model's split pattern is used: --encoder has no\n"
                 "                              effect then.  One HIP device; vocabularies up to 16,777,216, beyond the 16-bit\n"
                 "                              slot format on 32-bit tokens (a model without a split pattern replays one\n"
                 "                              pass per merge it already has)\n"
                 "  --input-list TEXT           With --train, instead of --input: a file with one path per line, each file one\n"
                 "                              piece of the corpus, optionally followed by a tab and a repeat count (the piece\n"
                 "                              is counted that many times); blank lines are skipped.  The pieces are read one\n"
                 "                              at a time, their chunks counted on the HIP device, and the training runs on the\n"
                 "                              counts as with --dedup: the model of the pieces' chunks laid end to end.  Every\n"
                 "                              piece is split on its own, so cut files where a letter or digit is followed by\n"
                 "                              whitespace.  Combines with --device-split, --device-split-unicode,\n"
                 "                              --continue-from, -c and -w; with --input or without --train it is an error\n"
                 "  --count                     Count only: split the pieces of --input-list, count their chunks on the HIP device\n"
                 "                              and write the counts to --counts-out.  Nothing is trained and no model is\n"
                 "                              written.  Many runs, on many devices or machines, can each count a share of a\n"
                 "                              corpus; --train --counts trains on all of them.  Combines with --encoder,\n"
                 "                              --device, --device-split, --device-split-unicode and --counts; with --train,\n"
                 "                              --encode, --decode or --input it is an error\n"
                 "  --counts-out TEXT           With --count (required there): the file the counts are written to\n"
                 "  --counts TEXT               With --train or --count, repeatable: counts written by --count, merged in the\n"
                 "                              order given before any --input-list pieces.  --train --counts a --counts b is\n"
                 "                              the model of --train --input-list over all the pieces behind a and b, in that\n"
                 "                              order (given out of order: the same counts, but -c first sees the first\n"
                 "                              occurrences of that order); --count --counts ckpt --input-list rest continues\n"
                 "                              a counting run.  The counts must come from the same --encoder; a missing or\n"
                 "                              malformed file is an error.  Excludes --input.  The training itself runs on one\n"
                 "                              HIP device\n"
                 "  --token-counts-out TEXT     With --encode, instead of --output: count how often every token id is used and\n"
                 "                              write one line \"id count\" per id, ascending from 0, zero counts included; no\n"
                 "                              token file is written, and with --device-encode no token leaves the device.\n"
                 "                              Takes --input, or --input-list (one path per line, optionally a tab and a\n"
                 "                              repeat count: the file is counted that many times).  --device-encode,\n"
                 "                              --device-split, --device-split-unicode, --rank-order, --dedup, --dropout and\n"
                 "                              --seed mean what they mean for --encode; without --device-encode the host loop\n"
                 "                              counts.  With --output, or without --encode, it is an error\n"
                 "  --min-frequency INT         With --train: the training ends when the best pair left occurs less often than\n"
                 "                              this (0, the default: no such rule), with fewer merges than --vocab-size asks for\n"
                 "  --max-token-length INT      With --train: no new token is longer than this many bytes (0, the default: no\n"
                 "                              limit; else at least 2); pairs that would make one are never chosen, and the\n"
                 "                              training ends when no other pair is left.  The tokens of a --continue-from\n"
                 "                              model stay.  Either option trains one merge per pass over the corpus: combine\n"
                 "                              with --dedup (or --input-list), so that a pass runs over the distinct chunks.\n"
                 "                              Both combine with every other --train option; without --train they are an error\n";
}

}  // namespace

int main(int argc, char *argv[]) {
    std::string input_path, input_list_path, output_path, special_token_path, encoder = "gpt4", model_path = "./output.model",
                continue_from, byte_ranges_path, counts_out_path, token_counts_path;
    std::vector<std::string> counts_paths;
    std::string conflict_resolution_str = "first";
    bool train = false, decode = false, encode = false, write_vocab = false, verbose = false, device_encode = false,
         device_decode = false, device_split = false, split_unicode = false, rank_order = false, dedup = false,
         count = false;
    int vocab_size = 512, device = 0;
    long long min_frequency = 0, max_token_length = 0;
    bool have_limits = false;
    double dropout = 0.0;
    bool have_dropout = false;
    unsigned long long seed = 0;

    // option parsing (the reference uses CLI11, :93-133)
    for (int i = 1; i < argc; ++i) {
        std::string arg = argv[i], val;
        bool has_val = false;
        size_t eq = arg.find('=');
        if (arg.rfind("--", 0) == 0 && eq != std::string::npos) { val = arg.substr(eq + 1); arg = arg.substr(0, eq); has_val = true; }
        auto value = [&](std::string *dst) -> bool {
            if (has_val) { *dst = val; return true; }
            if (i + 1 >= argc) { std::cerr << arg << ": 1 required TEXT missing\n"; return false; }
            *dst = argv[++i];
            return true;
        };
        std::string tmp;
        if (arg == "-h" || arg == "--help") { usage(); return 0; }
        else if (arg == "-i" || arg == "--input") { if (!value(&input_path)) return 106; }
        else if (arg == "--input-list") { if (!value(&input_list_path)) return 106; }
        else if (arg == "-o" || arg == "--output") { if (!value(&output_path)) return 106; }
        else if (arg == "-s" || arg == "--special-tokens-path") { if (!value(&special_token_path)) return 106; }
        else if (arg == "-m" || arg == "--model-path") { if (!value(&model_path)) return 106; }
        else if (arg == "--encoder") { if (!value(&encoder)) return 106; }
        else if (arg == "--continue-from") { if (!value(&continue_from)) return 106; }
        else if (arg == "--byte-ranges-out") { if (!value(&byte_ranges_path)) return 106; }
        else if (arg == "--counts-out") { if (!value(&counts_out_path)) return 106; }
        else if (arg == "--token-counts-out") { if (!value(&token_counts_path)) return 106; }
        else if (arg == "--counts") { if (!value(&tmp)) return 106; counts_paths.push_back(tmp); }
        else if (arg == "--vocab-size") {
            if (!value(&tmp)) return 106;
            try { vocab_size = std::stoi(tmp); } catch (...) { std::cerr << "--vocab-size: invalid integer " << tmp << "\n"; return 104; }
        } else if (arg == "--device") {
            if (!value(&tmp)) return 106;
            try { device = std::stoi(tmp); } catch (...) { std::cerr << "--device: invalid integer " << tmp << "\n"; return 104; }
        } else if (arg == "--min-frequency" || arg == "--max-token-length") {
            const std::string name = arg;
            if (!value(&tmp)) return 106;
            size_t used = 0;
            long long v = 0;
            try { v = std::stoll(tmp, &used); } catch (...) { used = 0; }
            if (used == 0 || used != tmp.size()) { std::cerr << name << ": invalid integer " << tmp << "\n"; return 104; }
            (name == "--min-frequency" ? min_frequency : max_token_length) = v;
            have_limits = true;
        } else if (arg == "--dropout") {
            if (!value(&tmp)) return 106;
            size_t used = 0;
            try { dropout = std::stod(tmp, &used); } catch (...) { used = 0; }
            if (used == 0 || used != tmp.size()) { std::cerr << "--dropout: invalid number " << tmp << "\n"; return 104; }
            have_dropout = true;
        } else if (arg == "--seed") {
            if (!value(&tmp)) return 106;
            size_t used = 0;
            try { seed = std::stoull(tmp, &used); } catch (...) { used = 0; }
            if (used == 0 || used != tmp.size() || tmp[0] == '-') { std::cerr << "--seed: invalid integer " << tmp << "\n"; return 104; }
        } else if (arg == "-c" || arg == "--conflict-resolution") {
            if (!value(&conflict_resolution_str)) return 106;
            if (conflict_resolution_str != "first" && conflict_resolution_str != "lexical") {   // CLI::IsMember, :129-131
                std::cerr << "--conflict-resolution: " << conflict_resolution_str << " not in {first,lexical}\n";
                return 105;
            }
        } else if (arg == "-t" || arg == "--train") train = true;
        else if (arg == "-d" || arg == "--decode") decode = true;
        else if (arg == "-e" || arg == "--encode") encode = true;
        else if (arg == "-w" || arg == "--write-vocab") write_vocab = true;
        else if (arg == "--device-encode") device_encode = true;
        else if (arg == "--device-decode") device_decode = true;
        else if (arg == "--device-split") device_split = true;
        else if (arg == "--device-split-unicode") device_split = split_unicode = true;
        else if (arg == "--rank-order") rank_order = true;
        else if (arg == "--dedup") dedup = true;
        else if (arg == "--count") count = true;
        else if (arg == "-v" || arg == "--verbose") verbose = true;
        else { std::cerr << "The following argument was not expected: " << arg << "\n"; return 109; }
    }

    uint64_t drop_threshold = 0;
    if (have_dropout) {
        if (mbpe_dropout_threshold(dropout, &drop_threshold) != MBPE_OK) {
            std::cerr << "--dropout: " << dropout << " not in [0, 1]\n";
            return 105;
        }
        if (!rank_order) { std::cerr << "--dropout requires --rank-order\n"; return 107; }
    }

    if (have_limits && !train) { std::cerr << "--min-frequency and --max-token-length require --train\n"; return 107; }

    if (!token_counts_path.empty() && (!encode || train || decode)) { std::cerr << "--token-counts-out requires --encode\n"; return 107; }
    if (!token_counts_path.empty() && !output_path.empty()) { std::cerr << "--token-counts-out excludes --output\n"; return 107; }
    if (!token_counts_path.empty() && !byte_ranges_path.empty()) { std::cerr << "--token-counts-out excludes --byte-ranges-out\n"; return 107; }
    if (count && (train || encode || decode)) { std::cerr << "--count excludes --train, --encode and --decode\n"; return 107; }
    if (count && counts_out_path.empty()) { std::cerr << "--count requires --counts-out\n"; return 107; }
    if (!counts_out_path.empty() && !count) { std::cerr << "--counts-out requires --count\n"; return 107; }
    if (!counts_paths.empty() && !train && !count) { std::cerr << "--counts requires --train or --count\n"; return 107; }
    if (!counts_paths.empty() && !input_path.empty()) { std::cerr << "--counts excludes --input\n"; return 107; }
    if (count && !input_path.empty()) { std::cerr << "--count takes --input-list, not --input\n"; return 107; }
    for (const std::string &c : counts_paths)
        if (!exists(c)) { std::cerr << "Counts file " << c << " does not exist\n"; return -1; }

    struct Piece { std::string path; uint32_t repeat; };
    std::vector<Piece> pieces;
    if (!input_list_path.empty()) {
        if (!input_path.empty()) { std::cerr << "--input-list excludes --input\n"; return 107; }
        if (!train && !count && token_counts_path.empty()) {
            std::cerr << "--input-list requires --train, --count or --token-counts-out\n";
            return 107;
        }
        if (!exists(input_list_path)) { std::cerr << "Input file " << input_list_path << " does not exist\n"; return -1; }
        std::ifstream list(input_list_path);
        for (std::string line; std::getline(list, line);) {
            if (!line.empty() && line.back() == '\r') line.pop_back();
            if (line.empty()) continue;
            Piece p{line, 1};
            const size_t tab = line.find('\t');
            if (tab != std::string::npos) {
                const std::string count = line.substr(tab + 1);
                size_t used = 0;
                unsigned long long v = 0;
                try { v = std::stoull(count, &used); } catch (...) { used = 0; }
                if (used == 0 || used != count.size() || count[0] == '-' || v == 0 || v > 0xFFFFFFFFull) {
                    std::cerr << "--input-list: invalid repeat count " << count << " for " << line.substr(0, tab) << "\n";
                    return 104;
                }
                p = Piece{line.substr(0, tab), static_cast<uint32_t>(v)};
            }
            if (!exists(p.path)) { std::cerr << "Input file " << p.path << " does not exist\n"; return -1; }
            pieces.push_back(p);
        }
    } else if (!input_path.empty()) {                           // :135-144
        if (!exists(input_path)) { std::cerr << "Input file " << input_path << " does not exist\n"; return -1; }
    } else if (counts_paths.empty()) {
        std::cerr << "Input file not specified\n";
        return -1;
    }

    std::string special_tokens_data;                            // :147-159
    bool have_special = false;
    if (!special_token_path.empty() && exists(special_token_path)) {
        std::string err;
        if (load_file_to_string(special_token_path, &special_tokens_data, &err)) {
            have_special = true;
            std::cout << "Loaded special tokens from " << special_token_path << "\n";
        } else {
            std::cerr << "Failed to load special tokens from " << special_token_path << ": " << err << "\n";
        }
    }

    auto t1 = std::chrono::high_resolution_clock::now();

    const char *pat = mbpe_split_pattern(encoder.c_str());       // :167-177
    if (!pat) { std::cout << "Encoder should be one of: basic, gpt2 or gpt4\n"; return -1; }

    mbpe_tokenizer *rt = nullptr;                               // Tokenizer rt(split_pattern), :179
    if (mbpe_tok_create(pat, &rt) != MBPE_OK) {
        std::cerr << "Error: " << mbpe_last_error() << "\n";
        return -1;
    }
    int rc = 0;
    if (train && !continue_from.empty() &&
        (!exists(continue_from) || mbpe_tok_load(rt, continue_from.c_str(), verbose) != MBPE_OK)) {
        std::cerr << "Model file " << continue_from << " does not exist or could not be loaded\n";
        mbpe_tok_destroy(rt);
        return -1;
    }
    if (train && have_limits && mbpe_tok_set_train_limits(rt, min_frequency, max_token_length) != MBPE_OK) {
        std::cerr << "Error: " << mbpe_last_error() << "\n";
        mbpe_tok_destroy(rt);
        return 105;
    }
    // --counts and --input-list: opens the pieces session, merges the counts files in the order given, then reads the
    // pieces one at a time.  false: a file could not be used (said on stderr; counts_failed for a counts file);
    // *trc: the code of the library call that failed, if one did
    bool counts_failed = false;
    auto feed_session = [&](int *trc) -> bool {
        std::string data, err;
        if (split_unicode) mbpe_tok_set_split_unicode(rt, 1);
        *trc = mbpe_tok_train_pieces_begin(rt, device, device_split);
        for (size_t k = 0; k < counts_paths.size() && *trc == MBPE_OK; ++k) {
            if (verbose) std::cout << "Loading counts " << counts_paths[k] << "\n";
            if (!load_file_to_string(counts_paths[k], &data, &err)) {
                std::cerr << "Failed to load counts file " << counts_paths[k] << ": " << err << "\n";
                return !(counts_failed = true);
            }
            if (mbpe_tok_train_pieces_merge(rt, reinterpret_cast<const uint8_t *>(data.data()), data.size()) != MBPE_OK) {
                std::cerr << "Counts file " << counts_paths[k] << " was refused: " << mbpe_last_error() << "\n";
                return !(counts_failed = true);
            }
        }
        for (size_t k = 0; k < pieces.size() && *trc == MBPE_OK; ++k) {
            if (verbose) std::cout << "Loading file " << pieces[k].path << "\n";
            if (!load_file_to_string(pieces[k].path, &data, &err)) {
                std::cerr << "Failed to load training input file: " << err << "\n";
                return false;
            }
            *trc = mbpe_tok_train_pieces_add(rt, reinterpret_cast<const uint8_t *>(data.data()), data.size(), pieces[k].repeat);
        }
        return true;
    };
    if (train) {                                                // :181-211
        if (have_special) mbpe_tok_set_special_tokens(rt, special_tokens_data.data(), special_tokens_data.size());
        else std::cout << "No special tokens file provided\n";
        const std::string &named = !input_list_path.empty() ? input_list_path : !input_path.empty() ? input_path : counts_paths[0];
        std::cout << "Training using file \"" << named << "\" encoder " << encoder << " vocab size " << vocab_size
                  << " model path " << model_path << "\n";
        const int cr = conflict_resolution_str == "lexical" ? 1 : 0;
        std::string input, err;
        if (!input_list_path.empty() || !counts_paths.empty()) {
            // the corpus in pieces: counts made earlier first, then one file in memory at a time, its chunks counted on
            // the device
            int trc = MBPE_OK;
            const bool read_ok = feed_session(&trc);
            if (!read_ok) {
                mbpe_tok_train_pieces_abort(rt);
                if (counts_failed) rc = -1;
            } else {
                if (verbose && trc == MBPE_OK) std::cout << "Starting training...\n";
                if (trc == MBPE_OK)
                    trc = mbpe_tok_train_pieces_finish(rt, (uint32_t)vocab_size, cr, verbose, !continue_from.empty());
                if (trc != MBPE_OK) {
                    std::cerr << "Error: " << mbpe_last_error() << "\n";
                    mbpe_tok_train_pieces_abort(rt);
                    rc = -1;
                } else {
                    mbpe_tok_save(rt, model_path.c_str(), write_vocab);
                }
            }
        } else {
            if (verbose) std::cout << "Loading file " << input_path << "\n";
            if (load_file_to_string(input_path, &input, &err)) {
                if (verbose) std::cout << "Starting training...\n";
                if (split_unicode) mbpe_tok_set_split_unicode(rt, 1);
                if (dedup) mbpe_tok_set_train_dedup(rt, 1);
                const uint8_t *in = reinterpret_cast<const uint8_t *>(input.data());
                const int trc =
                    !continue_from.empty()
                        ? mbpe_tok_train_continue(rt, in, input.size(), (uint32_t)vocab_size, cr, verbose, device, device_split)
                        : (device_split ? mbpe_tok_train_split_device : mbpe_tok_train)(rt, in, input.size(),
                                                                                        (uint32_t)vocab_size, cr, verbose, device);
                if (trc != MBPE_OK) {
                    std::cerr << "Error: " << mbpe_last_error() << "\n";
                    rc = -1;
                } else {
                    mbpe_tok_save(rt, model_path.c_str(), write_vocab);
                }
            } else {
                std::cerr << "Failed to load training input file: " << err << "\n";
            }
        }
    } else if (count) {
        // the counting stage alone: nothing is trained and no model is written
        std::cout << "Counting chunks, encoder " << encoder << ", counts to " << counts_out_path << "\n";
        int trc = MBPE_OK;
        bool ok = feed_session(&trc);
        if (ok && trc != MBPE_OK) {
            std::cerr << "Error: " << mbpe_last_error() << "\n";
            ok = false;
        }
        uint64_t n = 0;
        std::vector<uint8_t> blob;
        if (ok) {
            trc = mbpe_tok_train_pieces_export_size(rt, &n);
            if (trc == MBPE_OK) {
                blob.resize(n);
                trc = mbpe_tok_train_pieces_export(rt, blob.data(), blob.size(), &n);
            }
            if (trc != MBPE_OK) {
                std::cerr << "Error: " << mbpe_last_error() << "\n";
                ok = false;
            }
        }
        mbpe_tok_train_pieces_abort(rt);
        if (ok) {
            std::ofstream file(counts_out_path, std::ios::binary);
            file.write(reinterpret_cast<const char *>(blob.data()), (std::streamsize)n);
            file.close();
            if (!file) {
                std::cerr << "Failed to write " << counts_out_path << "\n";
                ok = false;
            } else {
                std::cout << "Wrote " << n << " bytes of counts\n";
            }
        }
        if (!ok) rc = -1;
    } else if (encode && !token_counts_path.empty()) {
        // the token frequency table of the input, or of the pieces of --input-list with their repeat counts
        if (!exists(model_path)) { std::cerr << "Model file " << model_path << " does not exist\n"; mbpe_tok_destroy(rt); return -1; }
        std::cout << "Counting tokens, encoder " << encoder << " model path " << model_path << " counts to "
                  << token_counts_path << "\n";
        mbpe_tok_load(rt, model_path.c_str(), verbose);
        if (device_encode && device_split) mbpe_tok_set_encode_split(rt, 1);
        if (rank_order) mbpe_tok_set_encode_order(rt, 1);
        if (have_dropout) mbpe_tok_set_encode_dropout(rt, drop_threshold, seed);
        if (split_unicode) mbpe_tok_set_split_unicode(rt, 1);
        if (dedup && device_encode) mbpe_tok_set_encode_dedup(rt, 1);
        if (pieces.empty()) pieces.push_back(Piece{input_path, 1});
        uint64_t total = 0;
        for (size_t k = 0; k < pieces.size() && rc == 0; ++k) {
            std::string input, err;
            if (verbose) std::cout << "Loading file " << pieces[k].path << "\n";
            if (!load_file_to_string(pieces[k].path, &input, &err)) {
                std::cerr << "Failed with error: " << err << "\n";
                rc = -1;
                break;
            }
            const uint64_t doc_off[2] = {0, input.size()};
            uint64_t n = 0;
            if (mbpe_tok_count_tokens(rt, reinterpret_cast<const uint8_t *>(input.data()), doc_off, 1, verbose,
                                      device_encode ? device : -1, pieces[k].repeat, &n) != MBPE_OK) {
                std::cerr << "Error: " << mbpe_last_error() << "\n";
                rc = -1;
            }
            total += n * pieces[k].repeat;
        }
        if (rc == 0) {
            uint64_t n_ids = 0;
            mbpe_tok_token_counts(rt, nullptr, 0, &n_ids, nullptr);
            std::vector<uint64_t> table(n_ids);
            if (mbpe_tok_token_counts(rt, table.data(), n_ids, &n_ids, nullptr) != MBPE_OK) {
                std::cerr << "Error: " << mbpe_last_error() << "\n";
                rc = -1;
            } else {
                std::ofstream file(token_counts_path);
                for (uint64_t i = 0; i < n_ids; ++i) file << i << ' ' << table[i] << '\n';
                file.close();
                if (!file) { std::cerr << "Failed to write " << token_counts_path << "\n"; rc = -1; }
                else std::cout << "Counted " << total << " tokens, wrote " << n_ids << " ids\n";
            }
        }
    } else if (encode) {                                        // :212-242
        if (output_path.empty()) { std::cerr << "Output file not specified\n"; mbpe_tok_destroy(rt); return -1; }
        if (!exists(model_path)) { std::cerr << "Model file " << model_path << " does not exist\n"; mbpe_tok_destroy(rt); return -1; }
        std::cout << "Encoding input file \"" << input_path << "\" encoder " << encoder << " model path " << model_path
                  << " output to " << output_path << "\n";
        mbpe_tok_load(rt, model_path.c_str(), verbose);
        std::string input, err;
        if (load_file_to_string(input_path, &input, &err)) {
            std::vector<Token> encoded(input.size() + 1);
            uint64_t n = 0;
            const uint8_t *in = reinterpret_cast<const uint8_t *>(input.data());
            if (device_encode && device_split) mbpe_tok_set_encode_split(rt, 1);
            if (rank_order) mbpe_tok_set_encode_order(rt, 1);
            if (have_dropout) mbpe_tok_set_encode_dropout(rt, drop_threshold, seed);
            if (split_unicode) mbpe_tok_set_split_unicode(rt, 1);
            if (dedup && device_encode) mbpe_tok_set_encode_dedup(rt, 1);
            std::vector<uint64_t> ranges(byte_ranges_path.empty() ? 0 : 2 * encoded.size());
            const int erc = !byte_ranges_path.empty()
                                ? mbpe_tok_encode_byteoff(rt, in, input.size(), verbose, device_encode ? device : -1,
                                                          encoded.data(), ranges.data(), encoded.size(), &n)
                            : device_encode
                                ? mbpe_tok_encode_device(rt, in, input.size(), verbose, device, encoded.data(), encoded.size(), &n)
                                : mbpe_tok_encode(rt, in, input.size(), verbose, encoded.data(), encoded.size(), &n);
            if (erc != MBPE_OK) {
                std::cerr << "Error: " << mbpe_last_error() << "\n";
                rc = -1;
            } else {
                encoded.resize(n);
                std::cout << "Writing " << encoded.size() << " encoded tokens\n";
                if (save_encoding(output_path, encoded, &err)) std::cout << "Success\n";
                else std::cerr << "Failed with error: " << err << "\n";
                if (!byte_ranges_path.empty()) {
                    std::ofstream rf(byte_ranges_path);
                    for (uint64_t j = 0; j < n; ++j) rf << ranges[2 * j] << ' ' << ranges[2 * j + 1] << '\n';
                    if (!rf) { std::cerr << "Failed to write " << byte_ranges_path << "\n"; rc = -1; }
                }
            }
        } else {
            std::cerr << "Failed with error: " << err << "\n";
        }
    } else if (decode) {                                        // :243-258
        std::cout << "Decoding input file \"" << input_path << "\" encoder " << encoder << " model path " << model_path
                  << " output to " << output_path << "\n";
        mbpe_tok_load(rt, model_path.c_str(), verbose);
        std::vector<Token> input;
        std::string err;
        if (load_encoding(input_path, &input, &err)) {
            uint64_t n = 0;
            int drc = device_decode ? mbpe_tok_decode_device(rt, input.data(), input.size(), 0, device, nullptr, 0, &n)
                                    : mbpe_tok_decode(rt, input.data(), input.size(), 0, nullptr, 0, &n);
            std::string decoded(n, '\0');
            uint8_t *dst = reinterpret_cast<uint8_t *>(&decoded[0]);
            if (drc == MBPE_OK)
                drc = device_decode ? mbpe_tok_decode_device(rt, input.data(), input.size(), verbose, device, dst, n, &n)
                                    : mbpe_tok_decode(rt, input.data(), input.size(), verbose, dst, n, &n);
            if (drc != MBPE_OK) {
                std::cerr << "Error: " << mbpe_last_error() << "\n";
                rc = -1;
            } else {
                std::cout << "Writing " << decoded.size() << " decoded tokens to " << output_path << "\n";
                std::ofstream file(output_path);
                if (file) file << decoded;
            }
        } else {
            std::cerr << "Failed with error: " << err << "\n";
        }
    }
    mbpe_tok_destroy(rt);
    if (rc != 0) return rc;

    auto t2 = std::chrono::high_resolution_clock::now();       // :260-264
    auto ms_int = std::chrono::duration_cast<std::chrono::milliseconds>(t2 - t1).count();
    std::cout << "Execution time: " << ms_int / 1000.0 << " (s)" << std::endl;
    return 0;
}
