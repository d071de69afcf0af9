// Host orchestration of the BPE training hot path behind the C-ABI
// (include/mbpe.h).  Drives the kernels of kernels.hip on one HIP stream:
//
//   begin : pair-count scan -> pair table, widen -> slot stream, first argmax
//   step k: merge(best[k]) -> apply deltas -> argmax -> best[k+1]
//
// which is the loop of Tokenizer::train (reference Tokenizer.h:551-589) for
// CONFLICT_RESOLUTION::LEXICAL.  The chosen pair never leaves the device
// between steps (the merge kernel reads best[k] from HBM); the host only
// synchronises once per batch of merges for housekeeping: error flags,
// compaction of holes, growth of the pair table.
#include "mbpe.h"
#include "mbpe_dev.h"
#include "dev_pool.h"
#include "wide_run.h"
#include "train_plan.h"
#include "split.h"
#include "hip_host.h"

#include <dlfcn.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <chrono>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

using namespace mbpe;

namespace {

#define HIPCHK(expr) MBPE_HIP_CHECK(expr, false)

uint64_t round_up(uint64_t v, uint64_t m) { return (v + m - 1) / m * m; }

uint32_t next_pow2(uint64_t v) {
    uint64_t p = 1;
    while (p < v) p <<= 1;
    return (uint32_t)p;
}

// does a NUL-led chunk collapse to a single token?
bool stoi_parses(const uint8_t *s, uint64_t n) { long long v; return stoi_value(s, n, &v); }

template <typename T>
void dfree(T *&p) {
    if (p) { (void)hipFree(p); p = nullptr; }
}

}  // namespace

// ---- RCCL, bound at run time: the library loads and runs on one GPU without it ----
namespace {
struct Rccl {
    void *lib = nullptr;
    int (*GetUniqueId)(void *) = nullptr;
    int (*CommInitRank)(void **, int, ncclUniqueId, int) = nullptr;
    int (*CommDestroy)(void *) = nullptr;
    int (*AllReduce)(const void *, void *, size_t, int, int, void *, hipStream_t) = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
    bool ok = false;
    std::string why;
};

Rccl &rccl() {
    static Rccl r;
    static bool tried = false;
    if (tried) return r;
    tried = true;
    for (const char *n : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
        r.lib = dlopen(n, RTLD_NOW | RTLD_LOCAL);
        if (r.lib) break;
    }
    if (!r.lib) { r.why = "librccl.so.1 not found"; return r; }
#define MBPE_BIND(field, name) \
    r.field = reinterpret_cast<decltype(r.field)>(dlsym(r.lib, name)); \
    if (!r.field) { r.why = std::string("missing RCCL symbol ") + name; return r; }
    MBPE_BIND(GetUniqueId, "ncclGetUniqueId")
    MBPE_BIND(CommInitRank, "ncclCommInitRank")
    MBPE_BIND(CommDestroy, "ncclCommDestroy")
    MBPE_BIND(AllReduce, "ncclAllReduce")
    MBPE_BIND(GetErrorString, "ncclGetErrorString")
#undef MBPE_BIND
    r.ok = true;
    return r;
}
}  // namespace

// The exchanges of the sharded protocol, each named for what the ranks sum.  A begin, a one-merge step and a
// batch sequence are units of local parts with exchanges in between: phase_exchange() says what an exchange carries,
// continue_after() what follows it.
enum class Phase {
    None,
    BeginCounts,    // begin: the byte-pair tables, the rank edges, the pairs counted
    BeginFirst,     // begin, `first`: every rank's earliest tied pair
    StepDeltas,     // one-merge step: one pair's delta rows
    StepFirst,      // one-merge step, `first`: every rank's earliest tied pair
    SeqDeltas,      // batch sequence: the delta rows of the batch
    SeqEdges,       // batch sequence: the rank edges
};

struct Exchange { uint32_t *buf; size_t words; };

struct mbpe_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    int n_cus = 256;

    // corpus
    const uint8_t *d_text = nullptr;
    uint8_t *d_text_owned = nullptr;
    uint8_t *d_endmask = nullptr;
    uint64_t n_bytes = 0;
    uint64_t n_chunks = 0;
    bool chunked = false;
    uint64_t n_barriers = 0;     // chunk ends in the corpus (= barrier slots of the barrier layout)
    bool barrier = false;        // this training keeps the chunk ends as barrier slots (mbpe_dev.h: kBarrier)
    bool loaded = false;
    bool inert = false;          // whole corpus collapses to one token (NUL quirk, basic)
    bool weighted = false;       // chunks come with weights (mbpe_load_corpus_weighted): the training runs on 32-bit tokens
    uint32_t *d_weights = nullptr;   // ... one per end bit of the mask, in order
    uint64_t n_weights = 0;

    uint32_t *pc_scratch = nullptr;   // pair-count scan: per-workgroup histogram snapshots (kept for the context's life)
    uint32_t *pc_bp = nullptr;        // mbpe_pair_count_u8: the 65,536-entry result table, then the 64-bit sum of its bins
    void *first_state = nullptr;      // `first` tie-break scratch (training)
    uint32_t *xf = nullptr;           // `first` on a sharded stream: every rank's earliest tied pair (hdr_words, see k_first_publish)

    // slot stream
    uint16_t *tok[2] = {nullptr, nullptr};
    int cur = 0;
    uint64_t cap_slots = 0;      // allocated slots per buffer
    uint64_t n_slots = 0;        // physical slots in use (multiple of kTile)
    uint32_t n_tiles = 0;
    TileSum *sums = nullptr;     // live tile summaries
    TileSum *side = nullptr;     // staging for the tiles a merge pass changed
    uint32_t *chg = nullptr;     // bitmap of those tiles
    uint32_t *tile_list = nullptr;   // the same as a dense list (batch rewrite pass)
    SelList *sel = nullptr;          // candidates of the threshold selection
    uint32_t *run_in = nullptr;      // per tile: run of t before it, for (t,t) pairs (k_run_final)
    int seq_slot = -1;               // index of the sequence being enqueued within its group (opt_time_kernels)
    unsigned long long *offsets = nullptr;

    // pair table
    PairTable tab = {};
    uint32_t hcap = 0;
    DevCtl *ctl = nullptr;
    unsigned long long *best = nullptr;   // [n_target + 1]
    // exchange buffer of one merge: [header: m, adj, RankEdge x n_ranks][LR: L[x], R[x] interleaved]
    uint32_t *xb = nullptr;
    uint32_t hdr_words = 0;               // single-merge header: m, adj, RankEdge x n_ranks
    uint32_t hdrb_words = 0;              // batch header: m_j, ADJ
    uint32_t *hdr_m = nullptr, *hdr_adj = nullptr;   // inside xb
    uint32_t *LR = nullptr;               // xb + hdr_words + hdrb_words
    BatchState *bs = nullptr;
    uint32_t *xb0 = nullptr;              // begin: [bp 65,536][header][pairs counted: kPairCountWords limbs]
    uint32_t h_pcount[kPairCountWords] = {};   // (host source of this rank's limbs)
    uint32_t *dlog = nullptr;             // the delta log of a stream pass and its partition buffer (launch_log_consume),
    uint32_t *dpart = nullptr;            //   or NULL
    LogState *log_state = nullptr;
    RankEdge *d_left = nullptr, *d_right = nullptr;   // composed neighbours (multi-GPU)

    // training
    uint32_t vocab_size = 0;
    uint32_t n_target = 0;
    uint32_t k = 0;              // merges launched
    uint32_t n_valid = 0;        // merges known to be real (table was not empty)
    bool begun = false;
    bool exhausted = false;
    uint32_t n_prior = 0;        // merges this training started from (mbpe_train_begin_from): best[0 .. n_prior) holds them
    std::vector<unsigned long long> h_prior;   // ... as the begin uploads them: count field all ones (no count was observed)
    ResumeTally *tally = nullptr;              // ... and the tally of its pair count
    float ms_replay = 0;                       // ... and the device time of the encoder that replayed them
    double merges_per_seq = 0;   // measured over the last group of sequences (0: not known yet)
    uint32_t first_b = 0, first_s = 0;   // `first` mode: sequences / single-pair sequences seen since begin
    bool first_legacy = false;   // `first` mode: most batches were single pairs with a shared count (position tie-breaks):
                                 //   the rest of the run takes the leaner one-merge-per-pass loop
    DevCtl h_ctl = {};

    // multi-GPU
    int rank = 0, n_ranks = 1;
    bool comm_external = false;           // the caller performs the all-reduce
    void *nccl_comm = nullptr;
    Phase pending = Phase::None;          // external mode: the exchange the caller has been asked to make
    Exchange pending_x = {};              // ... its buffer and size (phase_exchange, asked once when the call suspends)
    uint32_t pending_target = 0;          // external mode: merge count the pending call runs up to

    // options
    int64_t opt_compact_den = 16;
    int64_t opt_batch = 16;         // sequences between two host synchronisations (compaction is decided there)
    int64_t opt_time_kernels = 0;   // HIP events around every merge kernel (bench.py)
    int64_t opt_force_exchange = 0; // run the multi-rank path (edges, exchange) even with one rank
    int64_t opt_hier_argmax = -1;   // -1 auto (by table size), 0 full scan, 1 hierarchical
    int64_t opt_multi_merge = 1;    // 1: several independent merges per stream pass (batch sequences)
    int64_t opt_max_batch = kBatchDefault;
    int64_t opt_fused_min = 24;     // batches of at least this many pairs take the fused pass
    bool opt_byte_table = true;         // batches of byte pairs use the byte x byte lookup table (tests turn it off)
    int64_t opt_sel_cap = kSelCap;      // candidate-list capacity (tests lower it to force the overflow path)
    int64_t opt_threshold_select = 1;   // 0: always select with the bound-walking kernel
    int64_t opt_dense_table = -1;   // -1 auto / 1: dense pair table when vocab <= 32,768; 0: always hashed
    int hot_possible = 1;           // may a batch of the next group of sequences hold a "frequent" pair (kernels' dc_wanted)?
    unsigned long long last_top = ~0ull;   // count of the latest merge the host has seen: bounds every later count
    int64_t opt_barrier = -1;       // chunk ends as barrier slots: -1 when the ids need 16 bits, 0 never, 1 always
    int64_t opt_first_batches = 0;  // `first` mode: 1 = pairs whose counts no other pair shares are merged in batches too
                                    //   (no faster on text: words make chains of pairs with one count)
    int64_t opt_first = 0;          // 1: `first` tie-break (insertion order, PairCount.h:65-74) instead of lexical
    int64_t opt_pc_repeat = 1;      // mbpe_pair_count_u8 without an output table: launches per call (timing)
    uint32_t k_upper = 0;           // host-side upper bound of the device's k_done
    int sel_attempts = 3;           // gather + pick attempts enqueued per selection (see train_steps_batched)
    uint32_t max_batch_eff = kBatchMax, adj_pitch = kBatchMax;   // (set by mbpe_train_begin: see begin_local)
    // multi-GPU: what the selection of the sequence in flight decided (k_done, k_limit, batch_n, commit_n of DevCtl),
    // read back while its stream pass runs, so that exactly the cells the batch can touch are exchanged
    uint32_t *h_seq = nullptr;      // pinned, 16 words: [0..3] the multi-GPU copy, [8..15] launch_seq_info's
    uint32_t *d_seq_info = nullptr; // 8 words of device memory for launch_seq_info
    int64_t opt_pair_cells = -1;    // one log record per match with byte neighbours (mbpe_dev.h: launch_log_consume): -1 for
                                    //   streams from 64 Mi slots on, 0 never, 1 always
    int64_t opt_log_cap = 0;        // records the delta log holds (0: from the stream's size) and records a wave reserves
    int64_t opt_log_chunk = 0;      //   at a time (0: kLogChunkDefault, less on a small log): tests reach the full log and
                                    //   the chunk refill with them
    LogState h_log = {};            // what mbpe_train_begin sets the device's LogState to
    int64_t opt_lockstep = -1;      // small corpora: the host waits for every selection and enqueues only the kernels that
                                    //   sequence needs (-1: when the stream is short enough, 0 never, 1 always)
    hipEvent_t ev_sel = nullptr;
    std::vector<hipEvent_t> kev;    // event pool for opt_time_kernels
    std::vector<hipEvent_t> kev_f;  // ... around the fused pass alone
    uint32_t *seq_flags = nullptr;  // per sequence of a group: 1 = a fused pass ran (opt_time_kernels)
    std::vector<uint32_t> h_seq_flags;

    // 32-bit continuation of a training whose vocabulary lies beyond the 16-bit slot format (wide.h, wide_run.h)
    bool wide = false;               // this training hands over to the 32-bit loop after n_target merges
    WideRun wr;                      // ... that loop's buffers and state (wr.active: it has done so)
    uint32_t vocab_total = 0;        // the caller's vocab_size (vocab_size is the 16-bit part's)
    uint32_t n_target_total = 0;     // vocab_total - 256
    int64_t opt_wide_from = -1;      // tests: hand over after this many merges whatever the vocabulary (-1: at the format's limit)
    int64_t opt_first_wide = 0;      // 1: a `first` training may continue on 32-bit tokens too (0: MBPE_ERR_VOCAB, as before)
    int64_t opt_resume_wide = 0;     // 1: mbpe_train_begin_from may continue on 32-bit tokens (0: MBPE_ERR_VOCAB, as before)
    int64_t opt_min_frequency = 0;   // stopping rules (wide.h), read by the next begin: either non-zero and the training runs
    int64_t opt_max_token_length = 0;   // on 32-bit tokens from its first new merge, like one on a weighted corpus
    bool wide_direct = false;        // the training began on 32-bit tokens (begin_wide_direct): no slot stream, no best[]
    std::vector<uint32_t> h_prior_raw;   // ... and its prior merges, (a, b) as given: their ids may need more than 16 bits

    mbpe_stats stats = {};
    DevPool pool;                    // the device buffers of the trainings (dev_pool.h)
};

namespace {

// what the 32-bit loop's calls get of the context
WideDev wide_dev(mbpe_ctx *c) { return WideDev{c->stream, c->ev0, c->ev1, c->pool, c->n_cus, c->stats}; }

int sync_ctl(mbpe_ctx *c) {
    HIPCHK(hipMemcpyAsync(&c->h_ctl, c->ctl, sizeof(DevCtl), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->cur = (int)(c->h_ctl.cur & 1u);      // a fused pass flips the live buffer on the device
#ifdef MBPE_DIAG
    if (getenv("MBPE_MERGE_DIAG") || getenv("MBPE_FUSED_DIAG")) c->h_ctl.err = 0;   // timing-only kernels break the counts
#endif
    if (c->h_ctl.err) {
        char buf[320];
        snprintf(buf, sizeof(buf), "device error flags 0x%x (1=pair table full, 2=negative count, 4=missing pair, "
                                   "8=a pair occurs 2^31 times or more, or the byte-pair counts do not add up to the "
                                   "pairs scanned (a count reached 2^32), 16=a stream pass was skipped, 32=delta log overflow)",
                 c->h_ctl.err);
        mbpe_host::set_last_error(buf);
        return MBPE_ERR_OVERFLOW;
    }
    return MBPE_OK;
}

// One group of sequences or steps between two host synchronisations: `enqueue` puts it on the stream, between the
// events that time it; then the device's state and error flags are read back (h_ctl is current afterwards).
template <typename Enqueue>
int timed_group(mbpe_ctx *c, Enqueue enqueue) {
    HIPCHK(hipEventRecord(c->ev0, c->stream));
    int rc = enqueue();
    if (rc != MBPE_OK) return rc;
    HIPCHK(hipEventRecord(c->ev1, c->stream));
    rc = sync_ctl(c);
    if (rc != MBPE_OK) return rc;
    HIPCHK(hipGetLastError());
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    c->stats.ms_steps += ms;
    return MBPE_OK;
}

// The slot stream's buffers and the hashed pair table: what the conversion to the 32-bit loop is done with, and what a
// training that ends gives back first.  (best[] holds the slot stream's merges and stays.)
void free_slot_stream(mbpe_ctx *c) {
    c->pool.free(c->tok[0]); c->pool.free(c->tok[1]);
    c->pool.free(c->sums); c->pool.free(c->side); c->pool.free(c->chg); c->pool.free(c->tile_list);
    c->pool.free(c->offsets);
    c->pool.free(c->tab.hslot); c->pool.free(c->tab.ekey); c->pool.free(c->tab.ecnt);
    c->pool.free(c->tab.bmax); c->pool.free(c->tab.smax);
    c->pool.free(c->xb); c->pool.free(c->dlog); c->pool.free(c->dpart);
    c->pool.free(c->log_state);
    c->pool.free(c->run_in);
    c->pool.free(c->first_state);             // (the slot stream's `first` scratch; the 32-bit loop has its own)
    c->LR = nullptr;
}

void free_training(mbpe_ctx *c) {
    free_slot_stream(c);
    c->pool.free(c->tab.cells);
    c->pool.free(c->ctl); c->pool.free(c->best); c->pool.free(c->xb0);
    c->pool.free(c->d_left); c->pool.free(c->d_right); c->pool.free(c->bs); c->pool.free(c->sel); c->pool.free(c->seq_flags);
    c->pool.free(c->xf);
    c->pool.free(c->tally);
    c->wr.release(c->pool);
    c->wide_direct = false;
    c->h_prior_raw.clear();
    c->pending = Phase::None;
    c->begun = false;
    c->k = c->n_valid = c->n_prior = 0;
    c->exhausted = false;
}

void free_corpus(mbpe_ctx *c) {
    dfree(c->d_text_owned);
    dfree(c->d_endmask);
    dfree(c->d_weights);
    c->n_weights = 0;
    c->weighted = false;
    c->d_text = nullptr;
    c->loaded = false;
}

// dense layout: one cell per possible pair, row pitch = vocab rounded up to a power of two
static inline bool dense_possible(const mbpe_ctx *c) { return c->vocab_size <= 32768; }
static inline bool use_dense(const mbpe_ctx *c) {
    if (!dense_possible(c)) return false;
    if (c->wide) return false;           // (the conversion to the 32-bit loop reads the hashed layout's entry arrays)
    return c->opt_dense_table != 0;      // -1 (auto) and 1: dense whenever the vocabulary allows it
}

int alloc_table_dense(mbpe_ctx *c) {
    uint32_t vshift = 8;
    while ((1u << vshift) < c->vocab_size) ++vshift;
    c->tab = {};
    c->tab.vshift = vshift;
    c->tab.ecap = 1u << (2 * vshift);                 // <= 2^30 cells
    const size_t cells = (size_t)1 << (2 * vshift);
    HIPCHK(c->pool.alloc(&c->tab.cells, cells * 4));
    HIPCHK(hipMemsetAsync(c->tab.cells, 0, cells * 4, c->stream));
    const size_t nb = (cells >> kBlockShift) + 2, ns = (cells >> (2 * kBlockShift)) + 2;
    HIPCHK(c->pool.alloc(&c->tab.bmax, nb * 8));
    HIPCHK(c->pool.alloc(&c->tab.smax, ns * 8));
    HIPCHK(hipMemsetAsync(c->tab.bmax, 0, nb * 8, c->stream));
    HIPCHK(hipMemsetAsync(c->tab.smax, 0, ns * 8, c->stream));
    return MBPE_OK;
}

int alloc_table(mbpe_ctx *c, uint32_t ecap) {
    c->tab.ecap = ecap;
    c->hcap = next_pow2((uint64_t)ecap * 2);
    c->tab.hmask = c->hcap - 1;
    HIPCHK(c->pool.alloc(&c->tab.hslot, (size_t)c->hcap * 8));
    HIPCHK(c->pool.alloc(&c->tab.ekey, (size_t)ecap * 4));
    HIPCHK(c->pool.alloc(&c->tab.ecnt, (size_t)ecap * 4));
    const size_t nb = ((size_t)ecap >> kBlockShift) + 2, ns = ((size_t)ecap >> (2 * kBlockShift)) + 2;
    HIPCHK(c->pool.alloc(&c->tab.bmax, nb * 8));
    HIPCHK(c->pool.alloc(&c->tab.smax, ns * 8));
    HIPCHK(hipMemsetAsync(c->tab.bmax, 0, nb * 8, c->stream));
    HIPCHK(hipMemsetAsync(c->tab.smax, 0, ns * 8, c->stream));
    launch_fill_u32(c->stream, reinterpret_cast<uint32_t *>(c->tab.hslot), (uint64_t)c->hcap * 2, 0xFFFFFFFFu);
    return MBPE_OK;
}

// entries a batch of `steps` merges can add at most: per merge one (x,X) per
// left neighbour id, one (X,y) per right neighbour id and (X,X)
uint64_t batch_headroom(const mbpe_ctx *c, uint32_t steps) {
    uint64_t per = 2ull * c->vocab_size + 1;
    return per * steps;
}

uint64_t table_cap_limit(const mbpe_ctx *c) {
    uint64_t v = c->vocab_size;
    uint64_t lim = v * v;                    // every possible pair
    if (lim > (1ull << 30)) lim = 1ull << 30;   // argmax hierarchy: 1024 super-blocks of 1024 x 1024 entries
    return std::max<uint64_t>(lim, 1024);
}

struct WallTimer {
    float *acc;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    explicit WallTimer(float *a) : acc(a) {}
    ~WallTimer() { *acc += std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
};

int grow_table(mbpe_ctx *c, uint64_t want) {
    if (c->tab.cells) return MBPE_OK;          // the dense layout holds every possible pair
    WallTimer timer(&c->stats.ms_grow_table);
    c->stats.n_table_grows++;
    uint64_t lim = table_cap_limit(c);
    uint64_t ecap = std::min<uint64_t>(std::max<uint64_t>(want, (uint64_t)c->tab.ecap * 4), lim);
    if (ecap <= c->tab.ecap) return MBPE_OK;   // already at the limit: cannot overflow
    PairTable old = c->tab;
    c->tab = {};
    int rc = alloc_table(c, (uint32_t)ecap);
    if (rc != MBPE_OK) return rc;
    uint32_t n = c->h_ctl.n_entries;
    HIPCHK(hipMemcpyAsync(c->tab.ekey, old.ekey, (size_t)n * 4, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->tab.ecnt, old.ecnt, (size_t)n * 4, hipMemcpyDeviceToDevice, c->stream));
    // the block bounds refer to entry indices, which do not change
    HIPCHK(hipMemcpyAsync(c->tab.bmax, old.bmax, (((size_t)old.ecap >> kBlockShift) + 2) * 8,
                          hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->tab.smax, old.smax, (((size_t)old.ecap >> (2 * kBlockShift)) + 2) * 8,
                          hipMemcpyDeviceToDevice, c->stream));
    launch_table_rehash(c->stream, c->tab, c->ctl);
    HIPCHK(hipStreamSynchronize(c->stream));
    c->pool.release(old.hslot); c->pool.release(old.ekey); c->pool.release(old.ecnt);
    c->pool.release(old.bmax); c->pool.release(old.smax);
    return MBPE_OK;
}

int ensure_pc_scratch(mbpe_ctx *c) {
    if (!c->pc_scratch) HIPCHK(hipMalloc(&c->pc_scratch, pair_count_scratch_bytes(c->n_cus)));
    return MBPE_OK;
}

int ensure_events(std::vector<hipEvent_t> &pool, size_t n) {
    while (pool.size() < n) {
        hipEvent_t e;
        HIPCHK(hipEventCreate(&e));
        pool.push_back(e);
    }
    return MBPE_OK;
}

// the chunk-end convention of the stream, as the launchers take it
inline uint32_t endbit_of(const mbpe_ctx *c) { return !c->chunked ? 0u : c->barrier ? kBarrier : kEndBit; }

inline bool is_multi(const mbpe_ctx *c) { return c->n_ranks > 1 || c->opt_force_exchange; }
inline bool is_limited(const mbpe_ctx *c) { return c->opt_min_frequency != 0 || c->opt_max_token_length != 0; }

// ---- launch interface (mbpe_dev.h: StreamView, BatchView) ----
// The builders below are the only places that read the context's stream and batch buffers for a launch.
// Which token buffer a view names first.  A batch sequence passes buffers 0 and 1 and lets ctl->cur decide (a fused pass
// flips the live buffer without the host knowing); everything outside the sequences passes the live buffer first.
enum TokOrder { kBuffers01, kLiveFirst };

StreamView stream_view(const mbpe_ctx *c, TokOrder order) {
    const int first = order == kLiveFirst ? c->cur : 0;
    const bool multi = is_multi(c);
    StreamView v = {};
    v.stream = c->stream;
    v.tok = c->tok[first], v.tok_other = c->tok[1 - first];
    v.sums = c->sums, v.side = c->side, v.n_tiles = c->n_tiles;
    v.chg = c->chg, v.tile_list = c->tile_list;
    v.run_in = c->run_in, v.run_part = c->offsets + c->n_tiles;
    v.ctl = c->ctl;
    v.left_edge = multi ? c->d_left : nullptr, v.right_edge = multi ? c->d_right : nullptr;
    v.rank = c->rank, v.n_ranks = std::max(1, c->n_ranks);
    v.endbit = endbit_of(c), v.n_cus = c->n_cus;
    return v;
}

BatchView batch_view(const mbpe_ctx *c) { return BatchView{c->bs, c->hdr_m, c->hdr_adj, c->LR, c->dlog, c->dpart, c->log_state}; }

int do_compact(mbpe_ctx *c) {
    // c->h_ctl must be current
    if (!c->n_tiles) return MBPE_OK;
    WallTimer timer(&c->stats.ms_compact);
    const int dst = 1 - c->cur;
    const StreamView v = stream_view(c, kLiveFirst);       // live buffer -> the other one
    launch_tile_scan(v, c->offsets);
    launch_compact_scatter(v, c->offsets);
    const uint64_t live = c->h_ctl.n_live;
    const uint64_t padded = std::max<uint64_t>(round_up(live, kTile), kTile);
    launch_fill_u16(c->stream, c->tok[dst] + live, padded - live, (uint16_t)kHole);
    c->cur = dst;
    c->n_slots = padded;
    c->n_tiles = (uint32_t)(padded / kTile);
    launch_summarize(stream_view(c, kLiveFirst));
    DevCtl patch = c->h_ctl;
    patch.removed_total = 0;
    HIPCHK(hipMemcpyAsync(&c->ctl->removed_total, &patch.removed_total, sizeof(patch.removed_total),
                          hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(&c->ctl->cur), c->cur, 1, c->stream));
    c->h_ctl.cur = (uint32_t)c->cur;
    HIPCHK(hipStreamSynchronize(c->stream));
    c->h_ctl.removed_total = 0;
    c->stats.n_compactions++;
    return MBPE_OK;
}

}  // namespace

namespace mbpe_host {
int ctx_device(const mbpe_ctx *c) { return c->device; }
}  // namespace mbpe_host

extern "C" {

int mbpe_create(int device_id, mbpe_ctx **out) {
    if (!out) { mbpe_host::set_last_error("mbpe_create: out is NULL"); return MBPE_ERR_ARG; }
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0 || device_id < 0 || device_id >= n) {
        mbpe_host::set_last_error("no usable HIP device (the MI355X path has no CPU fallback)");
        return MBPE_ERR_NO_DEVICE;
    }
    HIPCHK(hipSetDevice(device_id));
    mbpe_ctx *c = new mbpe_ctx();
    c->device = device_id;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_id) == hipSuccess) c->n_cus = prop.multiProcessorCount;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_sel, hipEventDisableTiming) != hipSuccess ||
        hipHostMalloc(reinterpret_cast<void **>(&c->h_seq), 64, hipHostMallocDefault) != hipSuccess) {
        mbpe_host::set_last_error("could not create HIP stream / events");
        delete c;
        return MBPE_ERR_HIP;
    }
    *out = c;
    return MBPE_OK;
}

void mbpe_destroy(mbpe_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    free_training(c);
    c->pool.trim();
    free_corpus(c);
    dfree(c->pc_scratch);
    dfree(c->pc_bp);
    if (c->nccl_comm && rccl().ok) rccl().CommDestroy(c->nccl_comm);
    for (hipEvent_t e : c->kev) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->kev_f) (void)hipEventDestroy(e);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->ev_sel) (void)hipEventDestroy(c->ev_sel);
    if (c->h_seq) (void)hipHostFree(c->h_seq);
    dfree(c->d_seq_info);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

int mbpe_set_option(mbpe_ctx *c, const char *name, int64_t value) {
    if (!c || !name) return MBPE_ERR_ARG;
    std::string n(name);
    if (n == "compact_den") c->opt_compact_den = value;
    else if (n == "batch") c->opt_batch = std::max<int64_t>(1, value);
    else if (n == "time_kernels") c->opt_time_kernels = value;
    else if (n == "force_exchange") c->opt_force_exchange = value;
    else if (n == "hier_argmax") c->opt_hier_argmax = value;
    else if (n == "multi_merge") c->opt_multi_merge = value;
    else if (n == "max_batch") c->opt_max_batch = std::min<int64_t>(std::max<int64_t>(1, value), kBatchMax);
    else if (n == "fused_min") c->opt_fused_min = std::max<int64_t>(2, value);
    else if (n == "dense_table") c->opt_dense_table = value;
    else if (n == "threshold_select") c->opt_threshold_select = value != 0;
    else if (n == "conflict_resolution") {
        if (value != 0 && value != 1) { mbpe_host::set_last_error("conflict_resolution: 0 = first, 1 = lexical"); return MBPE_ERR_ARG; }
        // (only while a training is under way: a finished one, or one whose table ran empty, can be followed by
        //  another mbpe_train_begin on the same corpus with the other tie-break)
        if (c->begun && (c->pending != Phase::None || (c->k < c->n_target && !c->exhausted))) {
            mbpe_host::set_last_error("conflict_resolution cannot change in the middle of a training");
            return MBPE_ERR_STATE;
        }
        c->opt_first = value == 0;
    }
    else if (n == "chunk_barrier") c->opt_barrier = value < 0 ? -1 : value != 0;       // (read by the next mbpe_train_begin)
    else if (n == "first_batches") c->opt_first_batches = value != 0;
    else if (n == "sel_cap") c->opt_sel_cap = std::min<int64_t>(std::max<int64_t>(64, value), kSelCap);
    else if (n == "byte_table") c->opt_byte_table = value != 0;
    else if (n == "lockstep") c->opt_lockstep = value < 0 ? -1 : value != 0;
    else if (n == "pair_cells") c->opt_pair_cells = value < 0 ? -1 : value != 0;      // (read by the next mbpe_train_begin)
    else if (n == "log_cap") c->opt_log_cap = value < 0 ? 0 : std::min<int64_t>(value, 1ll << 29);       // (likewise; 0: default)
    else if (n == "log_chunk") c->opt_log_chunk = value < 0 ? 0 : std::min<int64_t>(value, 1ll << 16);   // (likewise)
    else if (n == "wide_from") c->opt_wide_from = value < 0 ? -1 : value;      // (read by the next mbpe_train_begin)
    else if (n == "first_wide") c->opt_first_wide = value != 0;                // (read by the next mbpe_train_begin)
    else if (n == "resume_wide") {                                             // (read by the next mbpe_train_begin_from)
        if (value != 0 && value != 1) { mbpe_host::set_last_error("resume_wide: 0 or 1"); return MBPE_ERR_ARG; }
        c->opt_resume_wide = value;
    }
    else if (n == "min_frequency") {                                           // (read by the next begin)
        if (value < 0 || value > 0x7FFFFFFFll) { mbpe_host::set_last_error("min_frequency: 0 (off) .. 2^31 - 1"); return MBPE_ERR_ARG; }
        c->opt_min_frequency = value;
    }
    else if (n == "max_token_length") {                                        // (likewise)
        if (value != 0 && (value < 2 || value > 0x7FFFFFFFll)) {
            mbpe_host::set_last_error("max_token_length: 0 (off), or 2 .. 2^31 - 1 bytes");
            return MBPE_ERR_ARG;
        }
        c->opt_max_token_length = value;
    }
    else if (n == "pc_repeat") c->opt_pc_repeat = std::min<int64_t>(std::max<int64_t>(1, value), 1000);
    else { mbpe_host::set_last_error("unknown option " + n); return MBPE_ERR_ARG; }
    return MBPE_OK;
}

// The two ends of a corpus load, shared by mbpe_load_corpus and mbpe_load_corpus_endmask.  load_reset: the old
// corpus goes, the new one's size and kind are noted.
static int load_reset(mbpe_ctx *c, uint64_t n_bytes, bool chunked, uint64_t n_chunks) {
    HIPCHK(hipSetDevice(c->device));
    free_training(c);
    free_corpus(c);
    // (the training buffers of a corpus of another size would not be handed out again: give them back before the
    //  new corpus is allocated, not only inside the next mbpe_train_begin)
    if (n_bytes != c->n_bytes || chunked != c->chunked) c->pool.trim();
    c->n_bytes = n_bytes;
    c->chunked = chunked;
    c->n_chunks = chunked ? n_chunks : 1;
    c->n_barriers = 0;
    c->barrier = false;
    c->inert = false;
    return MBPE_OK;
}

// load_finish: the text is taken in place or uploaded, the end mask of a chunked corpus (mask_bytes of it, on the
// side `mask_kind` says) copied into the context's own buffer; c->n_chunks is final by now.
static int load_finish(mbpe_ctx *c, const uint8_t *text, uint64_t n_bytes, int text_on_device, const uint8_t *mask,
                       size_t mask_bytes, hipMemcpyKind mask_kind) {
    const uint64_t n_vec = (n_bytes + 15) / 16;
    if (text_on_device) {
        c->d_text = text;
    } else {
        HIPCHK(hipMalloc(&c->d_text_owned, std::max<uint64_t>(n_vec * 16, 16)));
        if (n_bytes) HIPCHK(hipMemcpyAsync(c->d_text_owned, text, n_bytes, hipMemcpyHostToDevice, c->stream));
        c->d_text = c->d_text_owned;
    }
    if (mask) {
        HIPCHK(hipMalloc(&c->d_endmask, mask_bytes));
        HIPCHK(hipMemcpyAsync(c->d_endmask, mask, mask_bytes, mask_kind, c->stream));
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    c->loaded = true;
    c->stats = {};
    c->stats.n_bytes = n_bytes;
    c->stats.n_chunks = c->n_chunks;
    return MBPE_OK;
}

int mbpe_load_corpus(mbpe_ctx *c, const uint8_t *text, uint64_t n_bytes, const uint64_t *chunk_off,
                     uint64_t n_chunks, int text_on_device) {
    if (!c || (!text && n_bytes)) { mbpe_host::set_last_error("mbpe_load_corpus: NULL argument"); return MBPE_ERR_ARG; }
    const int rc0 = load_reset(c, n_bytes, chunk_off != nullptr, n_chunks);
    if (rc0 != MBPE_OK) return rc0;
    if (chunk_off) {
        if (chunk_off[0] != 0 || chunk_off[n_chunks] != n_bytes) {
            mbpe_host::set_last_error("chunk_off must start at 0 and end at n_bytes");
            return MBPE_ERR_ARG;
        }
        for (uint64_t i = 0; i < n_chunks; ++i)
            if (chunk_off[i] > chunk_off[i + 1]) {
                mbpe_host::set_last_error("chunk_off must be ascending");
                return MBPE_ERR_ARG;
            }
    }
    if (text_on_device && ((uintptr_t)text & 15)) {
        mbpe_host::set_last_error("device text must be 16-byte aligned");
        return MBPE_ERR_ARG;
    }

    // host view of the text for the NUL-quirk check (Tokenizer.h:86-93)
    std::vector<uint8_t> tmp;
    const uint8_t *h_text = text;
    if (text_on_device && n_bytes) {
        bool need_all = chunk_off != nullptr;
        uint64_t take = need_all ? n_bytes : std::min<uint64_t>(n_bytes, 64);
        tmp.resize(take);
        HIPCHK(hipMemcpy(tmp.data(), text, take, hipMemcpyDeviceToHost));
        h_text = tmp.data();
    }
    const uint64_t n_vec = (n_bytes + 15) / 16;
    std::vector<uint8_t> mask;
    if (chunk_off) {
        mask.assign(n_vec * 2 + 16, 0);
        uint64_t dropped = 0;
        for (uint64_t ci = 0; ci < n_chunks; ++ci) {
            uint64_t s = chunk_off[ci], e = chunk_off[ci + 1];
            if (e == s) continue;
            mask[(e - 1) >> 3] |= (uint8_t)(1u << ((e - 1) & 7));
            if (h_text[s] == 0 && stoi_parses(h_text + s + 1, e - s - 1)) {
                // collapses to one token in the reference: no pair ever starts or ends
                // inside it -> mark every byte as a chunk end so it stays inert
                for (uint64_t i = s; i < e; ++i) mask[i >> 3] |= (uint8_t)(1u << (i & 7));
                dropped++;
            }
        }
        c->n_chunks = n_chunks - dropped;
        uint64_t ends = 0;
        for (uint8_t b : mask) ends += (uint64_t)__builtin_popcount(b);
        c->n_barriers = ends;
    } else if (n_bytes && h_text[0] == 0) {
        // one chunk = whole text; stoi only looks at a prefix, 64 bytes are enough
        // to decide unless the prefix is all whitespace (then parse the host copy)
        uint64_t have = text_on_device ? tmp.size() : n_bytes;
        bool parses = stoi_parses(h_text + 1, have - 1);
        if (!parses && text_on_device && have < n_bytes) {
            bool all_ws = true;
            for (uint64_t i = 1; i < have; ++i)
                if (!(h_text[i] == ' ' || (h_text[i] >= 9 && h_text[i] <= 13))) { all_ws = false; break; }
            if (all_ws) {
                tmp.resize(n_bytes);
                HIPCHK(hipMemcpy(tmp.data(), text, n_bytes, hipMemcpyDeviceToHost));
                parses = stoi_parses(tmp.data() + 1, n_bytes - 1);
            }
        }
        c->inert = parses;
        if (parses) c->n_chunks = 0;
    }
    return load_finish(c, text, n_bytes, text_on_device, chunk_off ? mask.data() : nullptr, mask.size(),
                       hipMemcpyHostToDevice);
}

int mbpe_load_corpus_endmask(mbpe_ctx *c, const uint8_t *text, uint64_t n_bytes, int text_on_device,
                             const uint8_t *endmask_dev) {
    if (!c || (!text && n_bytes) || !endmask_dev) {
        mbpe_host::set_last_error("mbpe_load_corpus_endmask: NULL argument");
        return MBPE_ERR_ARG;
    }
    if ((text_on_device && ((uintptr_t)text & 15)) || ((uintptr_t)endmask_dev & 3)) {
        mbpe_host::set_last_error("device text must be 16-byte aligned, the end mask 4-byte aligned");
        return MBPE_ERR_ARG;
    }
    const int rc0 = load_reset(c, n_bytes, true, 0);
    if (rc0 != MBPE_OK) return rc0;
    // every set bit is a chunk end: the chunks, and the barrier slots of the barrier layout.  (A mask that carries
    // the NUL rule marks every byte of a collapsed chunk: like mbpe_load_corpus this counts those bytes as barriers;
    // the masks of mbpe_splitter_split hold no such chunk, see mbpe.h.)
    unsigned long long ends = 0;
    HIPCHK(read_scalar(c->stream, &ends, [&](unsigned long long *d) { launch_mask_popcount(c->stream, endmask_dev, n_bytes, d); }));
    c->n_chunks = ends;
    c->n_barriers = ends;
    return load_finish(c, text, n_bytes, text_on_device, endmask_dev, (n_bytes + 15) / 16 * 2 + 16,
                       hipMemcpyDeviceToDevice);
}

// The weights of a loaded chunked corpus, one per end bit of its mask: from here on the context trains weighted.
static int attach_weights(mbpe_ctx *c, const uint32_t *weights, uint64_t n_weights, hipMemcpyKind kind) {
    HIPCHK(hipMalloc(&c->d_weights, std::max<uint64_t>(n_weights, 1) * 4));
    if (n_weights) HIPCHK(hipMemcpyAsync(c->d_weights, weights, n_weights * 4, kind, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->n_weights = n_weights;
    c->weighted = true;
    return MBPE_OK;
}

static bool weight_ok(uint32_t w) { return w != 0u && w < 0x80000000u; }

int mbpe_load_corpus_weighted(mbpe_ctx *c, const uint8_t *text, uint64_t n_bytes, const uint64_t *chunk_off,
                              uint64_t n_chunks, int text_on_device, const uint32_t *weights) {
    if (!c || (!text && n_bytes) || !chunk_off || (!weights && n_chunks)) {
        mbpe_host::set_last_error("mbpe_load_corpus_weighted: NULL argument");
        return MBPE_ERR_ARG;
    }
    for (uint64_t i = 0; i < n_chunks; ++i)
        if (!weight_ok(weights[i])) {
            mbpe_host::set_last_error("mbpe_load_corpus_weighted: weight " + std::to_string(i) + " is 0, or 2^31 or more");
            return MBPE_ERR_ARG;
        }
    int rc = mbpe_load_corpus(c, text, n_bytes, chunk_off, n_chunks, text_on_device);
    if (rc != MBPE_OK) return rc;
    // One weight per end bit of the mask the load built: an empty chunk has none, a chunk the NUL rule made inert has
    // one per byte (every byte of it is a chunk end; no pair starts there, so the value never counts).
    std::vector<uint8_t> tmp;
    const uint8_t *h_text = text;
    if (text_on_device && n_bytes) {
        tmp.resize(n_bytes);
        HIPCHK(hipMemcpy(tmp.data(), text, n_bytes, hipMemcpyDeviceToHost));
        h_text = tmp.data();
    }
    std::vector<uint32_t> per_end;
    per_end.reserve(n_chunks);
    for (uint64_t ci = 0; ci < n_chunks; ++ci) {
        const uint64_t s = chunk_off[ci], e = chunk_off[ci + 1];
        if (e == s) continue;
        const bool inert = h_text[s] == 0 && stoi_parses(h_text + s + 1, e - s - 1);
        per_end.insert(per_end.end(), inert ? e - s : 1, weights[ci]);
    }
    if (per_end.size() != c->n_barriers) {
        mbpe_host::set_last_error("mbpe_load_corpus_weighted: the weights and the mask's chunk ends disagree");
        c->loaded = false;
        return MBPE_ERR_STATE;
    }
    rc = attach_weights(c, per_end.data(), per_end.size(), hipMemcpyHostToDevice);
    if (rc != MBPE_OK) c->loaded = false;
    return rc;
}

int mbpe_load_corpus_endmask_weighted(mbpe_ctx *c, const uint8_t *text, uint64_t n_bytes, int text_on_device,
                                      const uint8_t *endmask_dev, const uint32_t *weights, uint64_t n_weights,
                                      int weights_on_device) {
    if (!c || (!weights && n_weights)) {
        mbpe_host::set_last_error("mbpe_load_corpus_endmask_weighted: NULL argument");
        return MBPE_ERR_ARG;
    }
    if (weights_on_device && ((uintptr_t)weights & 3)) {
        mbpe_host::set_last_error("mbpe_load_corpus_endmask_weighted: device weights must be 4-byte aligned");
        return MBPE_ERR_ARG;
    }
    if (!weights_on_device)
        for (uint64_t i = 0; i < n_weights; ++i)
            if (!weight_ok(weights[i])) {
                mbpe_host::set_last_error("mbpe_load_corpus_endmask_weighted: weight " + std::to_string(i) +
                                          " is 0, or 2^31 or more");
                return MBPE_ERR_ARG;
            }
    int rc = mbpe_load_corpus_endmask(c, text, n_bytes, text_on_device, endmask_dev);
    if (rc != MBPE_OK) return rc;
    auto refuse = [&](const std::string &msg) {
        free_corpus(c);
        mbpe_host::set_last_error(msg);
        return MBPE_ERR_ARG;
    };
    if (n_weights != c->n_barriers)
        return refuse("mbpe_load_corpus_endmask_weighted: " + std::to_string(n_weights) + " weights for a mask of " +
                      std::to_string(c->n_barriers) + " chunk ends");
    if (weights_on_device && n_weights) {
        uint32_t flag = 0;
        HIPCHK(read_scalar(c->stream, &flag, [&](uint32_t *d) { launch_wide_check_weights(c->stream, weights, n_weights, d); }));
        if (flag) return refuse("mbpe_load_corpus_endmask_weighted: a weight is 0, or 2^31 or more");
    }
    rc = attach_weights(c, weights, n_weights, weights_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice);
    if (rc != MBPE_OK) c->loaded = false;
    return rc;
}

int mbpe_load_corpus_ranges(mbpe_ctx *c, const uint8_t *text, uint64_t n_bytes, const uint64_t *starts,
                            const uint64_t *ends, uint64_t n_chunks, int text_on_device) {
    if (!c || (!text && n_bytes) || ((!starts || !ends) && n_chunks)) {
        mbpe_host::set_last_error("mbpe_load_corpus_ranges: NULL argument");
        return MBPE_ERR_ARG;
    }
    uint64_t pos = 0, packed = 0;
    bool tiled = true;
    for (uint64_t i = 0; i < n_chunks; ++i) {
        if (starts[i] < pos || ends[i] < starts[i] || ends[i] > n_bytes) {
            mbpe_host::set_last_error("chunk ranges must be ascending, disjoint and inside the text");
            return MBPE_ERR_ARG;
        }
        if (starts[i] != pos) tiled = false;
        pos = ends[i];
        packed += ends[i] - starts[i];
    }
    if (pos != n_bytes) tiled = false;
    std::vector<uint64_t> off(n_chunks + 1);
    if (tiled) {
        for (uint64_t i = 0; i < n_chunks; ++i) off[i] = starts[i];
        off[n_chunks] = n_bytes;
        return mbpe_load_corpus(c, text, n_bytes, off.data(), n_chunks, text_on_device);
    }
    // bytes between the chunks are skipped (Tokenizer.h:506-540): train on the chunks packed together
    std::vector<uint8_t> host_copy;
    const uint8_t *src = text;
    if (text_on_device) {
        HIPCHK(hipSetDevice(c->device));
        host_copy.resize(n_bytes);
        HIPCHK(hipMemcpy(host_copy.data(), text, n_bytes, hipMemcpyDeviceToHost));
        src = host_copy.data();
    }
    std::vector<uint8_t> buf(packed);
    uint64_t w = 0;
    for (uint64_t i = 0; i < n_chunks; ++i) {
        off[i] = w;
        memcpy(buf.data() + w, src + starts[i], ends[i] - starts[i]);
        w += ends[i] - starts[i];
    }
    off[n_chunks] = w;
    return mbpe_load_corpus(c, buf.data(), packed, off.data(), n_chunks, 0);
}

// the number of adjacent pairs the pair-count scan counts: every byte but the last of each chunk (the NUL-inert
// chunks' bytes are all chunk ends in the mask; a NUL-inert one-chunk corpus is not scanned at all)
static uint64_t pairs_scanned(const mbpe_ctx *c) {
    if (c->chunked) return c->n_bytes - c->n_barriers;
    return c->inert || c->n_bytes < 2 ? 0 : c->n_bytes - 1;
}

int mbpe_pair_count_u8(mbpe_ctx *c, uint32_t *table65536_out) {
    if (!c) return MBPE_ERR_ARG;
    if (!c->loaded) { mbpe_host::set_last_error("mbpe_pair_count_u8: no corpus loaded"); return MBPE_ERR_STATE; }
    if (c->weighted) { mbpe_host::set_last_error("mbpe_pair_count_u8: the corpus has chunk weights"); return MBPE_ERR_STATE; }
    HIPCHK(hipSetDevice(c->device));
    int rcs = ensure_pc_scratch(c);
    if (rcs != MBPE_OK) return rcs;
    if (!c->pc_bp) HIPCHK(hipMalloc(&c->pc_bp, 65536 * 4 + 16));
    uint32_t *bp = c->pc_bp;
    HIPCHK(hipMemsetAsync(bp, 0, 65536 * 4, c->stream));
    // ("pc_repeat" > 1: that many launches back to back between the two events -- the kernel's sustained duration
    //  without one event marker's overhead per launch; the table then holds that multiple of every count)
    const int reps = table65536_out ? 1 : (int)std::max<int64_t>(1, c->opt_pc_repeat);
    // (every dispatch also carries its own start / stop events -- hipExtLaunchKernelGGL -- so that the kernel's duration
    //  is known without the gap between two launches or the cost of a marker: ms_pair_count_kernel)
    rcs = ensure_events(c->kev, 2ull * reps);
    if (rcs != MBPE_OK) return rcs;
    HIPCHK(hipEventRecord(c->ev0, c->stream));
    if (!c->inert)
        for (int r = 0; r < reps; ++r)
            launch_pair_count_u8(c->stream, c->d_text, c->n_bytes, c->d_endmask, bp, c->n_cus, c->pc_scratch,
                                 c->kev[2 * r], c->kev[2 * r + 1]);
    HIPCHK(hipEventRecord(c->ev1, c->stream));
    // (a count of 2^32 or more wrapped its bin: the 64-bit sum of the bins is then not the number of pairs scanned.
    //  Outside ev0..ev1, so that ms_pair_count times the scan alone; not with "pc_repeat" > 1, whose table is a multiple)
    unsigned long long *sum_dev = reinterpret_cast<unsigned long long *>(bp + 65536);
    if (reps == 1) launch_pair_total(c->stream, bp, nullptr, 0, sum_dev, nullptr);
    hipError_t e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess && table65536_out) e = hipMemcpy(table65536_out, bp, 65536 * 4, hipMemcpyDeviceToHost);
    unsigned long long sum = 0;
    if (e == hipSuccess && reps == 1) e = hipMemcpy(&sum, sum_dev, 8, hipMemcpyDeviceToHost);
    if (e != hipSuccess) { mbpe_host::set_last_error(hip_err("pair count", e)); return MBPE_ERR_HIP; }
    if (reps == 1 && sum != pairs_scanned(c)) {
        mbpe_host::set_last_error("mbpe_pair_count_u8: the counts add up to " + std::to_string(sum) + " of " +
                                  std::to_string(pairs_scanned(c)) + " pairs: a pair occurs 2^32 times or more");
        return MBPE_ERR_OVERFLOW;
    }
    HIPCHK(hipEventElapsedTime(&c->stats.ms_pair_count, c->ev0, c->ev1));
    c->stats.ms_pair_count /= (float)reps;
    c->stats.ms_pair_count_kernel = 0;
    if (!c->inert && c->n_bytes >= 2) {
        float sum = 0;
        for (int r = 0; r < reps; ++r) {
            float km = 0;
            HIPCHK(hipEventElapsedTime(&km, c->kev[2 * r], c->kev[2 * r + 1]));
            sum += km;
        }
        c->stats.ms_pair_count_kernel = sum / (float)reps;
    }
    c->stats.pair_count_launches += (uint32_t)reps;
#ifdef MBPE_PC_STAMPS
    {   // diagnostic build: the phases of the last launch, per workgroup (k_pair_count_u8_fast's stamps, 10 ns units)
        std::vector<unsigned long long> st((size_t)c->n_cus * 16);
        HIPCHK(hipMemcpy(st.data(), reinterpret_cast<const char *>(c->pc_scratch) + (size_t)c->n_cus * 32768 * 4, st.size() * 8,
                         hipMemcpyDeviceToHost));
        unsigned long long t0 = ~0ull;
        for (int w = 0; w < c->n_cus; ++w) if (st[16 * w] && st[16 * w] < t0) t0 = st[16 * w];
        for (int k = 0; k < 16; ++k) {
            double lo = 1e30, hi = 0, sum = 0; int cnt = 0;
            for (int w = 0; w < c->n_cus; ++w) {
                if (!st[16 * w + k]) continue;
                const double us = (double)(st[16 * w + k] - t0) * 0.01;
                lo = std::min(lo, us); hi = std::max(hi, us); sum += us; ++cnt;
            }
            if (cnt) fprintf(stderr, "pc stamp %2d: min %8.2f avg %8.2f max %8.2f us (%d workgroups)\n", k, lo, sum / cnt, hi, cnt);
        }
    }
#endif
    return MBPE_OK;
}

// ---- training phases ---------------------------------------------------------
// begin    = begin_local -> [BeginCounts] -> begin_finish_a -> [BeginFirst -> the tie-break's pick] -> begin_end
// step     = step_local  -> [StepDeltas]  -> step_finish_a  -> [StepFirst  -> the tie-break's pick] -> k++
// sequence = seq_stage_a -> [SeqDeltas]   -> seq_stage_b    -> [SeqEdges]   -> seq_stage_c
// The *First exchanges exist with the `first` tie-break on a sharded stream only.  continue_after() is the one statement
// of what follows an exchange.  With one rank the exchanges are skipped, with RCCL they are all-reduces enqueued between
// the parts on the context's stream (finish_unit); in external mode the library stops at every exchange so that the
// caller can reduce the buffer (suspend, mbpe_comm_exchange_done).

// large tables: walk the block bounds instead of scanning every entry ("hier_argmax": -1 auto, 0 never, 1 always)
static inline bool use_hier(const mbpe_ctx *c) {
    if (c->opt_hier_argmax >= 0) return c->opt_hier_argmax != 0;
    if (c->tab.cells) return c->tab.ecap > (1u << 20);
    return c->h_ctl.n_entries > (1u << 20);
}

// words of xb0, all of which the begin exchanges: [bp 65,536][header][pairs counted: kPairCountWords limbs]
static size_t begin_exchange_words(const mbpe_ctx *c) { return 65536 + (size_t)c->hdr_words + kPairCountWords; }

// what a begin that continues from existing merges starts from instead of the bytes: the corpus as the rank-ordered
// encoder left it (device, bit 31 = last token of its chunk) and the merges that made it
struct ResumeSrc { const uint32_t *tok; uint64_t n_tok; const uint32_t *prior; uint32_t n_prior; };

static int count_token_pairs(mbpe_ctx *c, const ResumeSrc *rs, uint64_t want);

static int begin_local(mbpe_ctx *c, uint32_t vocab_size, const ResumeSrc *rs = nullptr) {
    free_training(c);
    c->vocab_size = vocab_size;
    c->n_target = vocab_size - 256;
    c->k = c->n_valid = c->n_prior = rs ? rs->n_prior : 0;
    c->exhausted = false;
    c->first_legacy = false;
    c->sel_attempts = 3;             // (the first selection of a training primes its threshold through attempts 1 and 2)
    c->merges_per_seq = 0;
    c->first_b = c->first_s = 0;

    const uint64_t n = rs ? rs->n_tok : c->inert ? 0 : c->n_bytes;      // tokens the stream starts with
    // barrier layout: written sparsely (byte i -> slot 2i, its barrier or a hole behind it) into a first buffer of
    // twice the size, squeezed into the second one below, and only then does the first one get its final size
    const uint64_t n_bar = c->barrier ? c->n_barriers : 0;
    const uint64_t dense_slots = std::max<uint64_t>(round_up(n + n_bar, kTile), kTile);
    c->n_slots = c->barrier ? std::max<uint64_t>(2 * round_up(n, kTile / 2), kTile) : dense_slots;
    c->cap_slots = dense_slots;
    if (c->n_slots / kTile > 0x0FFFFFF0ull) { mbpe_host::set_last_error("corpus shard too large"); return MBPE_ERR_ARG; }
    c->n_tiles = (uint32_t)(c->n_slots / kTile);
    c->hdr_words = exchange_header_words(c->n_ranks);
    // the largest batch this training selects: "max_batch", and with several ranks at most 1,024 pairs -- the ADJ block
    // (batch x batch) is part of what every sequence all-reduces
    c->max_batch_eff = (uint32_t)std::min<int64_t>(c->opt_max_batch, is_multi(c) ? 1024 : kBatchMax);
    c->adj_pitch = (uint32_t)round_up(std::max<uint32_t>(c->max_batch_eff, 64u), 64);
    c->hdrb_words = (batch_header_words(c->adj_pitch) + 3) / 4 * 4;
    HIPCHK(c->pool.alloc(&c->tok[0], c->n_slots * 2));
    HIPCHK(c->pool.alloc(&c->tok[1], c->cap_slots * 2));
    HIPCHK(c->pool.alloc(&c->sums, (size_t)c->n_tiles * sizeof(TileSum)));
    HIPCHK(c->pool.alloc(&c->side, (size_t)c->n_tiles * sizeof(TileSum)));
    HIPCHK(c->pool.alloc(&c->chg, ((size_t)c->n_tiles / 32 + 2) * 4));
    HIPCHK(c->pool.alloc(&c->tile_list, ((size_t)c->n_tiles + 64) * 4));
    HIPCHK(hipMemsetAsync(c->chg, 0, ((size_t)c->n_tiles / 32 + 2) * 4, c->stream));
    HIPCHK(c->pool.alloc(&c->offsets, ((size_t)c->n_tiles + tile_scan_scratch(c->n_tiles)) * 8));
    // (the LR rows of the largest batch THIS training can select: seq_stage_a clamps every batch to max_batch_eff, so a
    //  later, larger "max_batch" cannot reach beyond it.  2 x max_batch_eff x lr_pitch(vocab) words: 1.05 GB at the
    //  defaults with vocab 32,000, 262 MB with several ranks or "max_batch" 1024)
    const size_t xb_words = (size_t)c->hdr_words + c->hdrb_words + lr_words(vocab_size, c->max_batch_eff) + 8;
    const size_t xb0_words = begin_exchange_words(c);
    HIPCHK(c->pool.alloc(&c->xb, xb_words * 4));
    HIPCHK(c->pool.alloc(&c->xb0, xb0_words * 4));
    HIPCHK(hipMemsetAsync(c->xb, 0, xb_words * 4, c->stream));
    HIPCHK(hipMemsetAsync(c->xb0, 0, xb0_words * 4, c->stream));
    if (c->opt_pair_cells > 0 || (c->opt_pair_cells < 0 && c->n_slots >= (64ull << 20))) {
        // The delta log.  A pass writes at most one record per match, and the matches of a batch are at most half the
        // slots; the partition buffer is laid out by the pairs' counts, which can add up to as much.  Both are capped
        // where the benchmark's largest pass (4,096 pairs, 2.7e8 matches) still fits: a pass beyond the partition
        // buffer keeps its atomics, a wave that finds the log full does so for its remaining tiles.
        LogState &init = c->h_log;
        init = LogState{};
        const uint64_t half = c->n_slots / 2 + 1;
        uint64_t cap = c->opt_log_cap > 0 ? (uint64_t)c->opt_log_cap : std::min<uint64_t>(std::max<uint64_t>(half / 8, 1u << 20), 1u << 28);
        // (a chunk per wave of the pass: large ones waste their tails on a small log)
        uint64_t chunk = c->opt_log_chunk > 0 ? (uint64_t)c->opt_log_chunk : std::min<uint64_t>(kLogChunkDefault, cap / 8192);
        chunk = std::max<uint64_t>(kLogChunkMin, std::min<uint64_t>(chunk, 1u << 16) / kLogChunkMin * kLogChunkMin);
        cap = std::max<uint64_t>(chunk, std::min<uint64_t>(cap, 1u << 29) / chunk * chunk);
        init.cap = (uint32_t)cap;
        init.chunk = (uint32_t)chunk;
        init.part_cap = (uint32_t)std::min<uint64_t>(half, 1u << 29);
        HIPCHK(c->pool.alloc(&c->dlog, (size_t)init.cap * 4));
        HIPCHK(c->pool.alloc(&c->dpart, (size_t)init.part_cap * 4));
        HIPCHK(c->pool.alloc(&c->log_state, sizeof(LogState)));
        HIPCHK(hipMemcpyAsync(c->log_state, &init, sizeof(LogState), hipMemcpyHostToDevice, c->stream));
    }
    c->hdr_m = c->xb + c->hdr_words;
    c->hdr_adj = c->hdr_m + kBatchMax;
    c->LR = c->xb + c->hdr_words + c->hdrb_words;
    HIPCHK(c->pool.alloc(&c->bs, sizeof(BatchState)));
    HIPCHK(c->pool.alloc(&c->sel, sizeof(SelList)));
    HIPCHK(c->pool.alloc(&c->run_in, ((size_t)c->n_tiles + 64) * 4));
    HIPCHK(c->pool.alloc(&c->seq_flags, 4096 * 4 * 4));      // 4 words per sequence of a group (k_seq_finish)
    HIPCHK(hipMemsetAsync(c->bs, 0, sizeof(BatchState), c->stream));
    HIPCHK(hipMemsetAsync(c->seq_flags, 0, 4096 * 4 * 4, c->stream));
    if (c->opt_first) {
        HIPCHK(c->pool.alloc(&c->first_state, first_state_bytes()));
        launch_first_init(c->stream, c->first_state);
        if (is_multi(c)) {
            HIPCHK(c->pool.alloc(&c->xf, (size_t)c->hdr_words * 4));
            HIPCHK(hipMemsetAsync(c->xf, 0, (size_t)c->hdr_words * 4, c->stream));
        }
    }
    c->k_upper = c->k;
    HIPCHK(c->pool.alloc(&c->d_left, sizeof(RankEdge)));
    HIPCHK(c->pool.alloc(&c->d_right, sizeof(RankEdge)));
    HIPCHK(c->pool.alloc(&c->ctl, sizeof(DevCtl)));
    HIPCHK(c->pool.alloc(&c->best, ((size_t)c->n_target + 2) * 8));
    {
        DevCtl init = {};
        init.n_live = n + n_bar;         // every corpus byte (every token of a resumed stream) starts as one live token
        init.k_done = c->k;
        init.n_ranks = (uint32_t)std::max(1, c->n_ranks);
        init.first_mode = c->opt_first ? 1u : 0u;
        init.adj_pitch = c->adj_pitch;
        init.cells_on = c->dlog ? 1u : 0u;
        init.cells_min = c->opt_pair_cells > 0 ? 2u : kCellsMinBatch;      // (forced on: every batch, and for the whole run)
        c->h_ctl = init;
        HIPCHK(hipMemcpyAsync(c->ctl, &c->h_ctl, sizeof(DevCtl), hipMemcpyHostToDevice, c->stream));
    }
    HIPCHK(hipMemsetAsync(c->best, 0, ((size_t)c->n_target + 2) * 8, c->stream));
    if (c->k) {
        // the merges this training continues from, as best[] holds a merge: (count, ~key) with every count bit set --
        // mbpe_train_result reports that as -1, and as the latest count it rules nothing out (update_hot_possible)
        c->h_prior.resize(c->k);
        for (uint32_t i = 0; i < c->k; ++i)
            c->h_prior[i] = pack_best(-1, (rs->prior[2 * i] << 16) | rs->prior[2 * i + 1]);
        HIPCHK(hipMemcpyAsync(c->best, c->h_prior.data(), (size_t)c->k * 8, hipMemcpyHostToDevice, c->stream));
    }

    // Sized for 288 GB of HBM: one entry per 8 corpus bytes up front (12 bytes of table per entry
    // plus 16 of hash index), so that even a corpus whose pairs never repeat rarely has to grow
    // the table -- growing means multi-GB allocations and a rehash.
    uint64_t want = 65536 + 2 * batch_headroom(c, (uint32_t)c->opt_batch);
    want = std::max<uint64_t>(want, n / 8);
    want = std::min<uint64_t>(want, table_cap_limit(c));
    // (a resumed stream's hashed table is sized once its pairs are counted: count_token_pairs)
    int rc = use_dense(c) ? alloc_table_dense(c) : rs ? MBPE_OK : alloc_table(c, (uint32_t)want);
    if (rc != MBPE_OK) return rc;

    rc = ensure_pc_scratch(c);
    if (rc != MBPE_OK) return rc;
    c->pool.trim();        // what this run did not take over from the previous one goes back to the driver
    HIPCHK(hipEventRecord(c->ev0, c->stream));
    if (!rs && n >= 2) launch_pair_count_u8(c->stream, c->d_text, n, c->d_endmask, c->xb0, c->n_cus, c->pc_scratch);
    c->cur = 0;
    if (rs) launch_slots_from_tokens(c->stream, rs->tok, n, endbit_of(c), c->tok[0], c->n_slots);
    if (c->barrier) {
        if (!rs) launch_widen_barrier(c->stream, c->d_text, n, c->d_endmask, c->tok[0], c->n_slots);
        launch_summarize(stream_view(c, kLiveFirst));
        const double ms_compact = c->stats.ms_compact;
        rc = do_compact(c);                     // tok[0] -> tok[1]; n_slots / n_tiles are the dense ones from here on
        if (rc != MBPE_OK) return rc;
        c->stats.n_compactions--;               // (part of the set-up, not one of the run's compactions)
        c->stats.ms_compact = ms_compact;
        c->pool.free(c->tok[0]);
        c->pool.trim();
        HIPCHK(c->pool.alloc(&c->tok[0], c->cap_slots * 2));
    } else {
        if (!rs) launch_widen(c->stream, c->d_text, n, c->d_endmask, c->tok[0], c->n_slots);
        launch_summarize(stream_view(c, kLiveFirst));
    }
    if (rs) return count_token_pairs(c, rs, want);
    if (is_multi(c)) {
        uint32_t *hdr = c->xb0 + 65536;
        launch_rank_edge(stream_view(c, kLiveFirst), hdr);
        const uint64_t p = pairs_scanned(c);
        for (uint32_t i = 0; i < kPairCountWords; ++i) c->h_pcount[i] = (uint32_t)(p >> (16 * i)) & 0xFFFFu;
        HIPCHK(hipMemcpyAsync(hdr + c->hdr_words, c->h_pcount, sizeof(c->h_pcount), hipMemcpyHostToDevice, c->stream));
    }
    return MBPE_OK;
}

// The pair table of a resumed stream: a fresh count of its adjacent pairs (the counterpart of launch_pair_count_u8 +
// launch_pair_total + launch_table_init), then the first argmax.  Dense layout: counted into the cells, sealed in place.
// Hashed layout: counted into bins of the begin's own, whose census sizes the table (`want`: what a begin from bytes
// would allocate) before every distinct pair is inserted once; the one host round trip of this path.
static int count_token_pairs(mbpe_ctx *c, const ResumeSrc *rs, uint64_t want) {
    const uint32_t ids = 256 + rs->n_prior;
    HIPCHK(c->pool.alloc(&c->tally, sizeof(ResumeTally)));
    HIPCHK(hipMemsetAsync(c->tally, 0, sizeof(ResumeTally), c->stream));
    if (c->tab.cells) {
        launch_pair_count_tokens(c->stream, rs->tok, rs->n_tok, ids, c->tab, PairBins{nullptr, nullptr, 0}, c->tally, c->n_cus);
        launch_bins_seal_dense(c->stream, c->tab, ids, c->ctl, c->tally);
    } else {
        // at most one bin per position and per possible pair; twice that many slots
        const uint64_t most = std::min<uint64_t>(rs->n_tok, (uint64_t)ids * ids);
        if (most > (1ull << 30)) {
            mbpe_host::set_last_error("mbpe_train_begin_from: more than 2^30 pairs to count into the hashed table");
            return MBPE_ERR_OVERFLOW;
        }
        PairBins bins = {nullptr, nullptr, next_pow2(std::max<uint64_t>(2 * most, 1024)) - 1};
        const size_t slots = (size_t)bins.mask + 1;
        HIPCHK(c->pool.alloc(&bins.key, slots * 4));
        HIPCHK(c->pool.alloc(&bins.cnt, slots * 4));
        launch_fill_u32(c->stream, bins.key, slots, kEmptyKey);
        HIPCHK(hipMemsetAsync(bins.cnt, 0, slots * 4, c->stream));
        launch_pair_count_tokens(c->stream, rs->tok, rs->n_tok, ids, c->tab, bins, c->tally, c->n_cus);
        launch_bins_tally(c->stream, bins, c->tally);
        ResumeTally h = {};
        HIPCHK(hipMemcpyAsync(&h, c->tally, sizeof(h), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        int rc = MBPE_OK;
        if (h.distinct > table_cap_limit(c)) {
            mbpe_host::set_last_error("mbpe_train_begin_from: the stream holds more distinct pairs than the pair table can");
            rc = MBPE_ERR_OVERFLOW;
        }
        want = std::max<uint64_t>(want, (uint64_t)h.distinct + 2 * batch_headroom(c, (uint32_t)c->opt_batch));
        want = std::min<uint64_t>(want, table_cap_limit(c));
        if (rc == MBPE_OK) rc = alloc_table(c, (uint32_t)want);
        if (rc == MBPE_OK) launch_bins_insert(c->stream, bins, c->tab, c->ctl);
        c->pool.free(bins.key);          // (handed out again, if at all, to work enqueued behind the insert)
        c->pool.free(bins.cnt);
        if (rc != MBPE_OK) return rc;
        c->h_ctl.n_entries = h.distinct;      // (use_hier: the table's size, until sync_ctl reads it)
    }
    launch_resume_check(c->stream, c->tally, c->ctl);
    launch_argmax(c->stream, c->tab, c->ctl, c->best + c->k, use_hier(c));
    if (c->opt_first) launch_first_tiebreak(stream_view(c, kLiveFirst), c->tab, c->best + c->k, c->first_state, c->xf, 0, 0);
    return MBPE_OK;
}

// The stream kernels exist in a plain and a HOT instantiation (LDS cache for the count updates of a frequent
// pair) and the device decides which one works: top_count * 8192 >= n_live (dc_wanted in kernels.hip).  The
// maximal count never rises, and n_live falls by at most one count per merge, so for the next `merges` merges
// HOT stays impossible while top * 8192 < (n_live - merges * top) * ranks: then it is not even launched.
static void update_hot_possible(mbpe_ctx *c, unsigned long long top_count, uint64_t merges) {
    c->last_top = top_count;
    if (c->comm_external) { c->hot_possible = 1; return; }     // (the caller drives the sequences one by one)
    const unsigned long long live = c->h_ctl.n_live;
    const unsigned long long eaten = merges * top_count;
    c->hot_possible = !(live > eaten && top_count * 8192ull < (live - eaten) * (unsigned long long)std::max(1, c->n_ranks));
}

// `first` on a sharded stream: the position tie-break needs one more exchange (every rank's earliest tied pair), so the
// finish of a begin / of a step comes in two parts around it
static inline bool first_sharded(const mbpe_ctx *c) { return c->opt_first && is_multi(c); }

// The `first` tie-break behind an argmax that wrote *best.  seq 0: the one-merge loop (live buffer first); seq 1: inside a
// batch sequence (best is the array, buffers 0 / 1).  phase: 0 on one rank; 1 before and 2 after the exchange of c->xf.
static void first_tiebreak(mbpe_ctx *c, unsigned long long *best, int seq, int phase) {
    launch_first_tiebreak(stream_view(c, seq ? kBuffers01 : kLiveFirst), c->tab, best, c->first_state, c->xf, seq, phase);
}

static void begin_finish_a(mbpe_ctx *c) {
    const uint32_t endbit = endbit_of(c);
    // (a pair that occurs 2^32 times or more -- on one GPU, or summed over the ranks by the u32 all-reduce -- leaves a
    //  small count in its bin, which k_table_init cannot tell from a true one: the bins must add up to the pairs counted,
    //  the ranks' own ones and the pairs across their boundaries.  Every rank decides on the same reduced data.)
    if (is_multi(c)) {
        uint32_t *hdr = c->xb0 + 65536;
        launch_boundary_pairs(c->stream, c->xb0, hdr, c->n_ranks, endbit, hdr + c->hdr_words);
        launch_compose_edges(c->stream, hdr, c->rank, c->n_ranks, c->d_left, c->d_right);
        launch_pair_total(c->stream, c->xb0, hdr + c->hdr_words, 0, nullptr, c->ctl);
    } else {
        launch_pair_total(c->stream, c->xb0, nullptr, pairs_scanned(c), nullptr, c->ctl);
    }
    launch_table_init(c->stream, c->xb0, c->tab, c->ctl);
    launch_argmax(c->stream, c->tab, c->ctl, c->best, use_hier(c));
    if (c->opt_first) first_tiebreak(c, c->best, 0, first_sharded(c) ? 1 : 0);
}

static int begin_end(mbpe_ctx *c) {
    HIPCHK(hipEventRecord(c->ev1, c->stream));
    int rc = sync_ctl(c);
    if (rc != MBPE_OK) return rc;
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventElapsedTime(&c->stats.ms_begin, c->ev0, c->ev1));
    unsigned long long b0 = 0;
    HIPCHK(hipMemcpy(&b0, c->best + c->k, 8, hipMemcpyDeviceToHost));      // (k: the merges a resumed training starts from)
    c->exhausted = (b0 == 0);   // empty table: the reference loop breaks at once (Tokenizer.h:586-588)
    update_hot_possible(c, b0 >> 32, (uint64_t)std::max<int64_t>(c->opt_batch, 1) * kBatchMax);
    c->begun = true;
    c->stats.ms_steps = 0;
    return MBPE_OK;
}

static void step_local(mbpe_ctx *c, int ev_slot) {
    const StreamView v = stream_view(c, kLiveFirst);
    const bool multi = is_multi(c);
    if (ev_slot >= 0) (void)hipEventRecord(c->kev[2 * ev_slot], c->stream);
    launch_merge(v, batch_view(c), c->best + c->k, 256 + c->k, &c->ctl->m, 0, inst_any(true));
    if (ev_slot >= 0) (void)hipEventRecord(c->kev[2 * ev_slot + 1], c->stream);
    if (multi) {
        launch_patch_sums(v, c->best + c->k, 0);
        launch_rank_edge(v, c->xb);
    }
}

static void step_finish_a(mbpe_ctx *c) {
    const bool multi = is_multi(c);
    launch_apply(stream_view(c, kLiveFirst), batch_view(c), c->tab, c->best + c->k, 256 + c->k, multi ? c->xb : nullptr, 0);
    if (multi) launch_compose_edges(c->stream, c->xb, c->rank, c->n_ranks, c->d_left, c->d_right);
    launch_argmax(c->stream, c->tab, c->ctl, c->best + c->k + 1, use_hier(c));
    if (c->opt_first) first_tiebreak(c, c->best + c->k + 1, 0, first_sharded(c) ? 1 : 0);
}

// words of xb a sequence has to exchange: both headers + the LR rows of its n_pairs members, lr_pitch(ids) cells each
// (ids = 256 + merges done when the sequence started: the neighbours x that can occur)
static size_t exchange_words(const mbpe_ctx *c, uint32_t ids, uint32_t n_pairs) {
    return (size_t)c->hdr_words + c->hdrb_words + (size_t)lr_words(ids, n_pairs);
}

// k_done / batch_n of the sequence whose selection has been enqueued: copied to pinned memory behind it
static_assert(offsetof(DevCtl, batch_n) == offsetof(DevCtl, k_done) + 8 && offsetof(DevCtl, commit_n) == offsetof(DevCtl, k_done) + 12,
              "seq_info_enqueue copies k_done, k_limit, batch_n, commit_n as four consecutive words");
static int seq_info_enqueue(mbpe_ctx *c) {
    HIPCHK(hipMemcpyAsync(c->h_seq, &c->ctl->k_done, 16, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipEventRecord(c->ev_sel, c->stream));
    return MBPE_OK;
}
static int seq_info_wait(mbpe_ctx *c, uint32_t *ids, uint32_t *n_pairs) {
    HIPCHK(hipEventSynchronize(c->ev_sel));
    *ids = 256u + c->h_seq[0];
    *n_pairs = c->h_seq[2];
    return MBPE_OK;
}

// ---- batch sequences: select -> (single pair: fused merge | several pairs: scan, validate, rewrite) ----
// The merge counter lives on the device (ctl->k_done); the host only keeps an
// upper bound (k_upper) between synchronisations.

// (`first` mode decides between equal counts by stream position: batches only hold pairs whose counts nothing else
//  shares -- k_sel_pick, k_validate -- and a pair with a shared count goes alone, after the position tie-break)
static inline bool use_batches(const mbpe_ctx *c) {
    // (`first` on a sharded stream: one merge per pass, the position tie-break is an exchange of its own)
    return c->opt_multi_merge != 0 && (!c->opt_first || (c->opt_first_batches && !c->first_legacy && !is_multi(c)));
}

// Small corpora: a sequence is ~25 launches of which ~16 return at once (the device decides which stream kernel of which
// instantiation works), and at 4-5 us per dispatch those are a third of a 0.16 ms sequence (BASELINE config 3).  There the
// host waits for the selection's result -- one event wait per sequence, ~20 us -- and enqueues exactly the pass, the
// tables / the single-pair apply and the rewrite this sequence needs.
static constexpr uint64_t kLockstepSlots = 32ull << 20;
static inline bool use_lockstep(const mbpe_ctx *c) {
    if (is_multi(c) || c->opt_first) return false;
    if (c->opt_lockstep >= 0) return c->opt_lockstep != 0;
    return c->n_slots <= kLockstepSlots;
}

// what every selection of this training is asked for
static SelectArgs select_args(const mbpe_ctx *c) {
    SelectArgs a = {};
    a.sel = c->opt_threshold_select ? c->sel : nullptr;
    a.n_target = c->n_target, a.max_batch = std::min<uint32_t>((uint32_t)c->opt_max_batch, c->max_batch_eff);
    a.fused_min = (uint32_t)c->opt_fused_min, a.sel_cap = (uint32_t)c->opt_sel_cap, a.byte_table = c->opt_byte_table;
    return a;
}

// (per-sequence record of k_seq_finish, while the kernels are timed)
static uint32_t *seq_flags_of(const mbpe_ctx *c) { return c->seq_slot >= 0 ? c->seq_flags + 4 * c->seq_slot : nullptr; }

// grids of the per-batch kernels: sized for the cap while batches are large or unknown, for a few dozen pairs on
// text, where a sequence merges a handful -- they stride over what the batch really holds either way
static uint32_t batch_hint(const mbpe_ctx *c) {
    return c->merges_per_seq > 0 && c->merges_per_seq < 128.0 ? 256u : c->max_batch_eff;
}

// (lockstep excludes several ranks: the view's edges are null and its n_ranks is 1)
static int seq_lockstep(mbpe_ctx *c, int ev_slot, bool *nothing_left) {
    const StreamView v = stream_view(c, kBuffers01);
    const BatchView b = batch_view(c);
    const SelectArgs sa = select_args(c);
    *nothing_left = false;
    // The first gather + pick attempt alone; only when it did not choose the batch (a list that overflowed or came back
    // empty, an unprimed threshold: a few times per training) the other two and the bound-walking kernel follow, behind one
    // more wait -- five launches fewer for every other sequence.
    const bool stepwise = sa.sel != nullptr;
    launch_select_batch(v, b, c->tab, c->best, sa, stepwise ? 1 : c->sel_attempts, 0, !stepwise);
    if (!c->d_seq_info) HIPCHK(hipMalloc(&c->d_seq_info, 32));
    for (int round = 0;; ++round) {
        launch_seq_info(v, b, c->best, c->d_seq_info);
        HIPCHK(hipMemcpyAsync(c->h_seq + 8, c->d_seq_info, 32, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipEventRecord(c->ev_sel, c->stream));
        HIPCHK(hipEventSynchronize(c->ev_sel));
        if (!stepwise || round > 0 || c->h_seq[14] != 0) break;
        launch_select_batch(v, b, c->tab, c->best, sa, 3, 1, true);
    }
    const uint32_t batch_n = c->h_seq[9], fused = c->h_seq[10];
    const Inst w = inst_known(c->h_seq[11] != 0, c->h_seq[12] != 0);
    if (ev_slot >= 0) { (void)hipEventRecord(c->kev[2 * ev_slot], c->stream); (void)hipEventRecord(c->kev_f[2 * ev_slot], c->stream); }
    if (batch_n == 0) {                        // the merge limit is reached (or the table is empty): nothing to enqueue
        if (ev_slot >= 0) { (void)hipEventRecord(c->kev_f[2 * ev_slot + 1], c->stream); (void)hipEventRecord(c->kev[2 * ev_slot + 1], c->stream); }
        *nothing_left = true;
        return MBPE_OK;
    }
    if (batch_n == 1) {
        launch_merge(v, b, c->best, 0, &c->ctl->m, 1, w);
    } else {
        // (a batch with a (t,t) member: the runs of its token before every tile, which launch_merge computes in the
        //  ordinary enqueue-everything flow)
        if (w.tt) launch_run_lengths(v, b.bs, c->best, 1);
        launch_log_plan(v, b);
        if (fused) launch_fused_batch(v, b, w);
        else launch_scan_batch(v, b, w);
        launch_log_consume(v, b);
    }
    if (ev_slot >= 0) { (void)hipEventRecord(c->kev_f[2 * ev_slot + 1], c->stream); (void)hipEventRecord(c->kev[2 * ev_slot + 1], c->stream); }
    c->k_upper = std::min<uint32_t>(c->n_target, c->h_seq[8] + batch_n);
    const uint32_t id_upper = 256 + c->k_upper;
    if (batch_n == 1) {
        launch_apply(v, b, c->tab, c->best, id_upper, nullptr, 1);
    } else {
        launch_batch_tables(v, b, c->tab, id_upper, batch_n);
        launch_rewrite_marked(v, b, w);
        launch_patch_sums(v, c->best, 1);
    }
    launch_seq_finish(v, b, seq_flags_of(c));
    return MBPE_OK;
}

static int seq_stage_a(mbpe_ctx *c, int ev_slot) {       // up to the delta exchange
    const StreamView v = stream_view(c, kBuffers01);
    const BatchView b = batch_view(c);
    const Inst w = inst_any(c->hot_possible != 0);
    launch_select_batch(v, b, c->tab, c->best, select_args(c), c->sel_attempts);
    if (c->opt_first) first_tiebreak(c, c->best, 1, 0);
    if (is_multi(c)) {
        // (a failed copy or event would leave the PREVIOUS sequence's sizes in h_seq: this rank would then exchange a
        //  length its peers do not -- fail the call instead)
        const int rc = seq_info_enqueue(c);
        if (rc != MBPE_OK) return rc;
    }
    if (ev_slot >= 0) (void)hipEventRecord(c->kev[2 * ev_slot], c->stream);
    // (the [m, adj] of a single pair: with several ranks in the exchange header, which is summed over them)
    launch_merge(v, b, c->best, 0, is_multi(c) ? c->xb : &c->ctl->m, 1, w);
    launch_log_plan(v, b);
    launch_scan_batch(v, b, w);
    if (ev_slot >= 0) (void)hipEventRecord(c->kev_f[2 * ev_slot], c->stream);
    launch_fused_batch(v, b, w);
    // (the logged records become L / R counts before anything reads the rows: the exchange of several ranks, validation,
    //  apply.  Inside the events: the log's consumers are part of what the pass costs)
    launch_log_consume(v, b);
    if (ev_slot >= 0) {
        (void)hipEventRecord(c->kev_f[2 * ev_slot + 1], c->stream);
        (void)hipEventRecord(c->kev[2 * ev_slot + 1], c->stream);
    }
    return MBPE_OK;
}

static void seq_stage_b(mbpe_ctx *c) {                   // up to the edge exchange
    const StreamView v = stream_view(c, kBuffers01);
    const BatchView b = batch_view(c);
    c->k_upper = std::min<uint32_t>(c->n_target, c->k_upper + std::min<uint32_t>((uint32_t)c->opt_max_batch, c->max_batch_eff));
    const uint32_t id_upper = 256 + c->k_upper;
    launch_batch_tables(v, b, c->tab, id_upper, batch_hint(c));
    launch_apply(v, b, c->tab, c->best, id_upper, is_multi(c) ? c->xb : nullptr, 1);
    launch_rewrite_marked(v, b, inst_any(c->hot_possible != 0));      // (both instantiations: the host does not know the batch)
    launch_patch_sums(v, c->best, 1);
    launch_seq_finish(v, b, seq_flags_of(c));
    if (is_multi(c)) launch_rank_edge(v, c->xb);
}

static void seq_stage_c(mbpe_ctx *c) {                   // after the edge exchange
    if (is_multi(c)) launch_compose_edges(c->stream, c->xb, c->rank, c->n_ranks, c->d_left, c->d_right);
}

// ---- the sharded protocol: what an exchange carries, what follows it, and who makes it ----

// What the ranks sum in exchange p.  The only place that forms these sizes, for RCCL and for mbpe_comm_exchange_buffer,
// asked once per exchange by whoever issues it (finish_unit, suspend); SeqDeltas waits for the selection's result
// (seq_info_enqueue) and is what stats.exchanges / exchange_words count.
static int phase_exchange(mbpe_ctx *c, Phase p, Exchange *x) {
    switch (p) {
    case Phase::BeginCounts: *x = {c->xb0, begin_exchange_words(c)}; return MBPE_OK;
    case Phase::StepDeltas: *x = {c->xb, exchange_words(c, 256 + c->k, 1)}; return MBPE_OK;
    case Phase::SeqDeltas: {
        uint32_t ids = 0, n_pairs = 0;
        const int rc = seq_info_wait(c, &ids, &n_pairs);
        if (rc != MBPE_OK) return rc;
        *x = {c->xb, exchange_words(c, ids, n_pairs)};
        c->stats.exchange_words += x->words;
        c->stats.exchanges++;
        return MBPE_OK;
    }
    case Phase::SeqEdges: *x = {c->xb, c->hdr_words}; return MBPE_OK;
    case Phase::BeginFirst: case Phase::StepFirst: *x = {c->xf, c->hdr_words}; return MBPE_OK;
    case Phase::None: break;
    }
    *x = {};
    return MBPE_OK;
}

// Enqueues the part of a unit that follows exchange p; returns the unit's next exchange, or None when all of it is on the
// stream (what ends a unit -- begin_end, a step's k++, the host's synchronisation -- is its driver's).
static Phase continue_after(mbpe_ctx *c, Phase p) {
    switch (p) {
    case Phase::BeginCounts: begin_finish_a(c); return first_sharded(c) ? Phase::BeginFirst : Phase::None;
    case Phase::BeginFirst: first_tiebreak(c, c->best, 0, 2); return Phase::None;
    case Phase::StepDeltas: step_finish_a(c); return first_sharded(c) ? Phase::StepFirst : Phase::None;
    case Phase::StepFirst: first_tiebreak(c, c->best + c->k + 1, 0, 2); return Phase::None;
    case Phase::SeqDeltas: seq_stage_b(c); return Phase::SeqEdges;
    case Phase::SeqEdges: seq_stage_c(c); return Phase::None;
    case Phase::None: break;
    }
    return Phase::None;
}

static int comm_allreduce(mbpe_ctx *c, uint32_t *buf, size_t count);   // RCCL (below)

// One rank, or several over RCCL: everything of a unit behind its local part, whose first exchange is p.  With several
// ranks every exchange is an all-reduce on the context's stream; nothing here synchronises the host with the stream.
static int finish_unit(mbpe_ctx *c, Phase p) {
    for (; p != Phase::None; p = continue_after(c, p)) {
        if (!is_multi(c)) continue;
        Exchange x = {};
        int rc = phase_exchange(c, p, &x);
        if (rc == MBPE_OK) rc = comm_allreduce(c, x.buf, x.words);
        if (rc != MBPE_OK) return rc;
    }
    return MBPE_OK;
}

// External transport: the caller makes exchange p, and mbpe_comm_exchange_done continues behind it.
static int suspend(mbpe_ctx *c, Phase p) {
    HIPCHK(hipStreamSynchronize(c->stream));
    const int rc = phase_exchange(c, p, &c->pending_x);
    if (rc != MBPE_OK) return rc;
    c->pending = p;
    return MBPE_NEED_EXCHANGE;
}

// table entries one sequence can add at most
static uint64_t seq_headroom(const mbpe_ctx *c) {
    return (uint64_t)c->opt_max_batch * (2ull * c->vocab_size + kBatchMax + 1);
}

// sequences between two host synchronisations: bounded by the "batch" option and by
// the table headroom they need (8M entries at most)
static uint32_t seqs_per_sync(const mbpe_ctx *c) {
    if (c->tab.cells) return (uint32_t)std::min<int64_t>(4096, std::max<int64_t>(1, c->opt_batch));   // nothing to reserve
    uint64_t g = (8ull << 20) / seq_headroom(c);
    g = std::max<uint64_t>(1, std::min<uint64_t>(g, (uint64_t)c->opt_batch));
    return (uint32_t)g;
}

// housekeeping between batches: errors, holes, table headroom (h_ctl must be current)
static int after_batch(mbpe_ctx *c) {
    c->n_valid = c->k;
    if (c->opt_compact_den > 0 && c->h_ctl.removed_total > 0 &&
        c->h_ctl.removed_total * (uint64_t)c->opt_compact_den >= c->n_slots) {
        int rc = do_compact(c);
        if (rc != MBPE_OK) return rc;
    }
    return MBPE_OK;
}

// room for `entries` more entries in the pair table (h_ctl.n_entries must be current); the dense table has a cell for
// every possible pair
static int reserve_table(mbpe_ctx *c, uint64_t entries) {
    const uint64_t need = (uint64_t)c->h_ctl.n_entries + entries;
    if (c->tab.cells || need <= c->tab.ecap) return MBPE_OK;
    return grow_table(c, need * 2);
}

// The chosen pair `pair` occurs nowhere.  Merging it changes neither the stream nor the table, so the reference chooses
// it again and again (its loop only ends on an empty table, Tokenizer.h:586-588; PairCountLexicalOrder never erases):
// the merges k .. target of this call are that pair, written to best[] from `from` on without their passes.  Batch
// sequences count their merges on the device (set_k_done); a one-merge step is told its index.
static int fill_zero_tail(mbpe_ctx *c, unsigned long long pair, uint32_t from, uint32_t target, bool set_k_done) {
    if (target > c->k) {
        std::vector<unsigned long long> rest(target - c->k, pair);
        HIPCHK(hipMemcpy(c->best + from, rest.data(), rest.size() * 8, hipMemcpyHostToDevice));
    }
    if (set_k_done) {
        HIPCHK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(&c->ctl->k_done), (int)target, 1, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        c->h_ctl.k_done = target;
    }
    c->k = target;
    return MBPE_OK;
}

// External transport: the local part of the next sequence (or merge) of an mbpe_train_steps call, up to its first exchange.
static int start_unit_external(mbpe_ctx *c, bool batched) {
    int rc = reserve_table(c, batched ? seq_headroom(c) : batch_headroom(c, 1));
    if (rc != MBPE_OK) return rc;
    if (!batched) {
        step_local(c, -1);
        return suspend(c, Phase::StepDeltas);
    }
    c->k_upper = c->k;
    rc = seq_stage_a(c, -1);
    if (rc != MBPE_OK) return rc;
    return suspend(c, Phase::SeqDeltas);
}

int mbpe_merges_check(const uint32_t *merges, uint32_t n_merges) {
    if (!merges && n_merges) { mbpe_host::set_last_error("mbpe_merges_check: merges is NULL"); return MBPE_ERR_ARG; }
    std::unordered_map<unsigned long long, uint32_t> seen;
    seen.reserve(n_merges);
    for (uint32_t k = 0; k < n_merges; ++k) {
        const uint32_t a = merges[2 * k], b = merges[2 * k + 1];
        if (a >= 256ull + k || b >= 256ull + k) {
            mbpe_host::set_last_error("merge " + std::to_string(k) + ": (" + std::to_string(a) + ", " + std::to_string(b) +
                                      ") names a token that does not exist before it (ids below " +
                                      std::to_string(256ull + k) + ")");
            return MBPE_ERR_ARG;
        }
        const auto ins = seen.emplace(((unsigned long long)a << 32) | b, k);
        if (!ins.second) {
            mbpe_host::set_last_error("merge " + std::to_string(k) + ": the pair (" + std::to_string(a) + ", " +
                                      std::to_string(b) + ") is merge " + std::to_string(ins.first->second) + " already");
            return MBPE_ERR_ARG;
        }
    }
    return MBPE_OK;
}

// The replay of mbpe_train_begin_from: the loaded corpus through a temporary rank-ordered encoder, which reads the
// context's text and end mask where they are.  *tok_out: n_bytes u32 of device memory of the call's own (the caller
// frees it), holding *n_tok_out flagged tokens.  The encoder is gone before the training buffers are allocated.
static int replay_prior(mbpe_ctx *c, const uint32_t *prior, uint32_t n_prior, uint32_t **tok_out, uint64_t *n_tok_out) {
    *tok_out = nullptr;
    *n_tok_out = 0;
    c->ms_replay = 0;
    const uint64_t n = c->inert ? 0 : c->n_bytes;
    if (!n) return MBPE_OK;
    free_training(c);        // (the peak of a resumed begin is the replay: nothing of an earlier training stays beside it)
    c->pool.trim();
    uint8_t *own_mask = nullptr;
    mbpe_encoder *enc = nullptr;
    auto run = [&]() -> int {
        const uint8_t *mask = c->d_endmask;
        if (!mask) {         // one chunk = the whole text: a mask with its last byte marked
            const size_t mask_bytes = (n + 15) / 16 * 2 + 16;
            const uint8_t bit = (uint8_t)(1u << ((n - 1) & 7));
            HIPCHK(hipMalloc(&own_mask, mask_bytes));
            HIPCHK(hipMemsetAsync(own_mask, 0, mask_bytes, c->stream));
            HIPCHK(hipMemcpyAsync(own_mask + ((n - 1) >> 3), &bit, 1, hipMemcpyHostToDevice, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
            mask = own_mask;
        }
        HIPCHK(hipMalloc(tok_out, n * 4));
        int rc = mbpe_encoder_create(c->device, prior, n_prior, &enc);
        if (rc == MBPE_OK) rc = mbpe_encoder_set_option(enc, "rank_order", 1);
        if (rc == MBPE_OK)
            rc = mbpe_encoder_encode_endmask(enc, c->d_text, n, mask, nullptr, 0, nullptr, 0, *tok_out, n, 32, 1, nullptr,
                                             n_tok_out, nullptr);
        if (rc == MBPE_OK) rc = mbpe_encoder_kernel_ms(enc, &c->ms_replay);
        return rc;
    };
    const int rc = run();
    const std::string keep = rc == MBPE_OK ? std::string() : std::string(mbpe_last_error());
    mbpe_encoder_destroy(enc);
    dfree(own_mask);
    if (rc != MBPE_OK) {
        dfree(*tok_out);
        mbpe_host::set_last_error(keep);
    }
    return rc;
}

// A training that begins on 32-bit tokens (Route::WideDirect): one on a corpus with chunk weights or under a stopping
// rule, from merge n_prior on (0 included: an empty prior table leaves the bytes as tokens), and one continued from so
// many merges that no slot stream can hold their ids.  The replay's tokens are the 32-bit stream (WideRun::begin_from):
// no slot stream, no best[].
static int begin_wide_direct(mbpe_ctx *c, uint32_t vocab_size, const uint32_t *prior, uint32_t n_prior) {
    uint32_t *tok = nullptr;
    uint64_t n_tok = 0;
    int rc = replay_prior(c, prior, n_prior, &tok, &n_tok);
    if (rc != MBPE_OK) return rc;
    free_training(c);
    c->vocab_size = 256 + n_prior;           // (the slot stream's share: the prior merges, all of them made already)
    c->n_target = c->k = c->n_valid = c->n_prior = c->k_upper = n_prior;
    c->vocab_total = vocab_size;
    c->n_target_total = vocab_size - 256;
    c->exhausted = false;
    c->barrier = false;                      // (32-bit tokens carry their chunk ends as flags)
    c->wide = true;
    c->wide_direct = true;
    c->h_ctl = DevCtl{};
    c->h_prior_raw.assign(prior, prior + 2 * (size_t)n_prior);
    const WideTokens src = {&tok, n_tok, c->ms_replay, prior, n_prior, vocab_size, c->weighted ? c->d_weights : nullptr,
                            c->n_weights, c->opt_min_frequency, c->opt_max_token_length};
    rc = c->wr.begin_from(wide_dev(c), src, WideGoal{vocab_size - 256 - n_prior, 256 + n_prior, c->opt_first != 0});
    if (rc == MBPE_OK) {
        c->last_top = c->wr.top0;
        c->begun = true;
        c->pool.trim();
    } else {
        (void)hipStreamSynchronize(c->stream);
    }
    dfree(tok);
    return rc;
}

// Every begin, behind its entry point's argument checks: the route (train_plan.h), then the begin it names.
static int begin_routed(mbpe_ctx *c, uint32_t vocab_size, const uint32_t *prior, uint32_t n_prior) {
    const BeginPlan plan = plan_begin(BeginIn{c->chunked, c->opt_barrier, c->opt_first, c->opt_first_wide, c->opt_resume_wide,
                                              c->opt_wide_from, c->weighted, is_limited(c), is_multi(c), vocab_size, n_prior});
    if (plan.rc != MBPE_OK) return fail(plan.rc, plan.message);
    HIPCHK(hipSetDevice(c->device));
    if (plan.route == Route::WideDirect) return begin_wide_direct(c, vocab_size, prior, n_prior);
    c->barrier = plan.barrier;
    c->wide = plan.route == Route::SlotThenWide;      // (the slot stream's share ends at slot_vocab, where wide_convert takes over)
    if (!n_prior) {
        int rc = begin_local(c, plan.slot_vocab);
        c->vocab_total = vocab_size;
        c->n_target_total = vocab_size - 256;
        if (rc != MBPE_OK) return rc;
        if (is_multi(c) && c->comm_external) return suspend(c, Phase::BeginCounts);
        rc = finish_unit(c, Phase::BeginCounts);
        if (rc != MBPE_OK) return rc;
        return begin_end(c);
    }
    uint32_t *tok = nullptr;
    uint64_t n_tok = 0;
    int rc = replay_prior(c, prior, n_prior, &tok, &n_tok);
    if (rc != MBPE_OK) return rc;
    auto rest = [&]() -> int {
        if (c->barrier && n_tok) {
            // the barrier slots the compaction keeps are the tokens' end flags: they must be the mask's end bits, by
            // which the stream is sized
            unsigned long long ends = 0;
            HIPCHK(read_scalar(c->stream, &ends, [&](unsigned long long *d) { launch_token_ends(c->stream, tok, n_tok, d); }));
            if (ends != c->n_barriers) {
                mbpe_host::set_last_error("mbpe_train_begin_from: the replay left " + std::to_string(ends) + " chunk ends, the "
                                          "corpus has " + std::to_string(c->n_barriers));
                return MBPE_ERR_STATE;
            }
        }
        const ResumeSrc rs = {tok, n_tok, prior, n_prior};
        int r = begin_local(c, plan.slot_vocab, &rs);
        c->vocab_total = vocab_size;
        c->n_target_total = vocab_size - 256;
        if (r != MBPE_OK) return r;
        r = begin_end(c);
        c->stats.ms_begin += c->ms_replay;
        return r;
    };
    rc = rest();
    (void)hipStreamSynchronize(c->stream);      // (the kernels that read the tokens are done)
    dfree(tok);
    c->pool.trim();
    return rc;
}

int mbpe_train_begin(mbpe_ctx *c, uint32_t vocab_size) {
    if (!c) return MBPE_ERR_ARG;
    if (!c->loaded) { mbpe_host::set_last_error("mbpe_train_begin: no corpus loaded"); return MBPE_ERR_STATE; }
    if (vocab_size < 256) { mbpe_host::set_last_error("vocab_size must be >= 256"); return MBPE_ERR_ARG; }
    return begin_routed(c, vocab_size, nullptr, 0);
}

int mbpe_train_begin_from(mbpe_ctx *c, uint32_t vocab_size, const uint32_t *prior_merges, uint32_t n_prior) {
    if (!c) return MBPE_ERR_ARG;
    if (n_prior == 0) return mbpe_train_begin(c, vocab_size);
    if (!c->loaded) { mbpe_host::set_last_error("mbpe_train_begin_from: no corpus loaded"); return MBPE_ERR_STATE; }
    if (vocab_size < 256) { mbpe_host::set_last_error("vocab_size must be >= 256"); return MBPE_ERR_ARG; }
    if (!prior_merges) { mbpe_host::set_last_error("mbpe_train_begin_from: prior_merges is NULL"); return MBPE_ERR_ARG; }
    if (n_prior > vocab_size - 256) {
        mbpe_host::set_last_error("mbpe_train_begin_from: " + std::to_string(n_prior) + " prior merges are more than vocab_size " +
                                  std::to_string(vocab_size) + " holds");
        return MBPE_ERR_ARG;
    }
    const int rc = mbpe_merges_check(prior_merges, n_prior);
    return rc != MBPE_OK ? rc : begin_routed(c, vocab_size, prior_merges, n_prior);
}

// the batch-sequence loop of mbpe_train_steps (one GPU, or several over RCCL)
// (max_seqs: stop after that many sequences, however many merges they committed)
static int train_steps_batched(mbpe_ctx *c, uint32_t n_steps, uint32_t *steps_done_out,
                               uint32_t max_seqs = 0xFFFFFFFFu) {
    const uint32_t start = c->k;
    const uint32_t target = (uint32_t)std::min<uint64_t>(c->n_target, (uint64_t)c->k + n_steps);
    HIPCHK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(&c->ctl->k_limit), (int)target, 1, c->stream));
    uint32_t seqs_left = max_seqs;
    while (c->k < target && !c->exhausted && seqs_left) {
        const uint32_t group = std::min<uint32_t>(seqs_per_sync(c), seqs_left);
        int rc = reserve_table(c, seq_headroom(c) * group);
        if (rc != MBPE_OK) return rc;
        if (c->opt_time_kernels) {
            rc = ensure_events(c->kev, 2ull * group);
            if (rc == MBPE_OK) rc = ensure_events(c->kev_f, 2ull * group);
            if (rc != MBPE_OK) return rc;
        }
        c->k_upper = c->k;
        // (for THIS group: the "batch" / "max_batch" options may have changed since the bound was last computed)
        update_hot_possible(c, c->last_top, (uint64_t)group * kBatchMax);
        const uint32_t batches_before = c->h_ctl.n_batches, singles_before = c->h_ctl.cut_single;
        unsigned long long live_prev = c->h_ctl.n_live;      // (exact: the host synchronised before this group)
        uint32_t launched = 0;
        rc = timed_group(c, [&]() -> int {
            // (sequences past the target do nothing on the device -- ctl->k_limit -- but cost their launches: enqueue
            //  as many as the last group's merges per sequence say are needed; before that is known, as many as are
            //  needed if every one merged max_batch pairs)
            const bool lockstep = use_lockstep(c);
            for (uint32_t g = 0; g < group && (lockstep || (c->merges_per_seq > 0 ? c->k + g * c->merges_per_seq < target : c->k_upper < target));
                 ++g, ++launched) {
                const int slot = c->opt_time_kernels ? (int)g : -1;
                c->seq_slot = slot;
                if (lockstep) {
                    bool nothing_left = false;
                    const int r = seq_lockstep(c, slot, &nothing_left);
                    if (r != MBPE_OK) return r;
                    if (nothing_left) {
                        // (no k_seq_finish ran for this slot: its record would be an earlier sequence's)
                        if (slot >= 0) HIPCHK(hipMemsetAsync(c->seq_flags + 4 * slot, 0, 16, c->stream));
                        ++launched;
                        break;
                    }
                    continue;
                }
                // (with several ranks the selection's result arrives while the stream pass runs: every rank took the same
                //  decisions, so the counts agree, and the all-reduce is enqueued long before the pass ends)
                int r = seq_stage_a(c, slot);
                if (r == MBPE_OK) r = finish_unit(c, Phase::SeqDeltas);
                if (r != MBPE_OK) return r;
            }
            c->seq_slot = -1;
            return MBPE_OK;
        });
        if (rc != MBPE_OK) return rc;
        if (c->opt_time_kernels) {
            c->h_seq_flags.resize(4 * (size_t)launched);
            if (launched)
                HIPCHK(hipMemcpy(c->h_seq_flags.data(), c->seq_flags, launched * 16, hipMemcpyDeviceToHost));
            for (uint32_t g = 0; g < launched; ++g) {
                float km = 0;
                HIPCHK(hipEventElapsedTime(&km, c->kev[2 * g], c->kev[2 * g + 1]));
                c->stats.ms_merge_kernel += km;
                const unsigned long long live_after =
                    ((unsigned long long)c->h_seq_flags[4 * g + 2] << 32) | c->h_seq_flags[4 * g + 1];
                if (c->h_seq_flags[4 * g]) {      // this sequence ran the fused pass
                    HIPCHK(hipEventElapsedTime(&km, c->kev_f[2 * g], c->kev_f[2 * g + 1]));
                    c->stats.ms_fused_kernel += km;
                    c->stats.fused_launches++;
                    c->stats.fused_slots += c->n_slots;
                    c->stats.fused_live_tokens += live_prev + live_after;
                }
                live_prev = live_after;
            }
            c->stats.merge_launches += c->h_ctl.n_batches - batches_before;   // sequences that did work
        }
        // (All three attempts of the selection, always.  Round 4 tried to enqueue the second and third only while the last
        //  group had needed one: a selection that then needs them falls back to the bound-walking kernel, whose batches are
        //  a few pairs -- with a host round trip per sequence 138 passes instead of 66 on the benchmark workload.)
        const uint32_t before = c->k;
        c->k = c->h_ctl.k_done;
        if (c->k) {             // the count of the latest merge bounds every later one
            unsigned long long last = 0;
            HIPCHK(hipMemcpy(&last, c->best + (c->k - 1), 8, hipMemcpyDeviceToHost));
            update_hot_possible(c, last >> 32, (uint64_t)seqs_per_sync(c) * kBatchMax);
            if ((last >> 32) == 0 && c->k < target && c->k != before) {      // every remaining merge of this call is that pair
                rc = fill_zero_tail(c, last, c->k, target, true);
                if (rc != MBPE_OK) return rc;
            }
        }
        rc = after_batch(c);
        if (rc != MBPE_OK) return rc;
        if (c->k == before) break;      // nothing left to merge
        seqs_left -= launched;
        c->merges_per_seq = std::max(1.0, (double)(c->k - before) / std::max(1u, launched));
        if (c->opt_first && c->k < c->n_target) {
            // `first` mode on data full of equal counts: nearly every sequence is one pair plus the position
            // tie-break, which the one-merge-per-pass loop does with fewer kernels.  Hand over: best[k] = the next
            // pair, chosen as that loop's step_finish would have
            c->first_b += c->h_ctl.n_batches - batches_before;
            c->first_s += c->h_ctl.cut_single - singles_before;
            if (c->first_b >= 32) {
                const bool hand_over = 2 * c->first_s > c->first_b;
                c->first_b = c->first_s = 0;
                if (!hand_over) continue;
                c->first_legacy = true;
                HIPCHK(hipMemsetAsync(c->best + c->k, 0, 8, c->stream));
                launch_argmax(c->stream, c->tab, c->ctl, c->best + c->k, use_hier(c));
                first_tiebreak(c, c->best + c->k, 0, 0);
                HIPCHK(hipStreamSynchronize(c->stream));
                break;
            }
        }
    }
    if (steps_done_out) *steps_done_out = c->k - start;
    return MBPE_OK;
}

static int train_steps16(mbpe_ctx *c, uint32_t n_steps, uint32_t *steps_done_out) {
    if (steps_done_out) *steps_done_out = 0;
    if (is_multi(c) && c->comm_external) {
        // one sequence (or one merge) per round trip: local part now, the rest in mbpe_comm_exchange_done
        if (n_steps == 0 || c->k >= c->n_target || c->exhausted) return MBPE_OK;
        c->pending_target = std::min<uint32_t>(c->n_target, c->k + n_steps);
        const bool batched = use_batches(c);
        if (batched)
            HIPCHK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(&c->ctl->k_limit), (int)c->pending_target, 1,
                                     c->stream));
        return start_unit_external(c, batched);
    }
    uint32_t done = 0;
    if (use_batches(c)) {
        int rc = train_steps_batched(c, n_steps, &done);
        if (rc != MBPE_OK || use_batches(c) || done >= n_steps) {      // (use_batches turns false when `first` mode hands over)
            if (steps_done_out) *steps_done_out = done;
            return rc;
        }
    }
    while (done < n_steps && c->k < c->n_target && !c->exhausted) {
        uint32_t batch = std::min<uint32_t>({(uint32_t)c->opt_batch, n_steps - done, c->n_target - c->k});
        int rc = reserve_table(c, batch_headroom(c, batch));   // (h_ctl.n_entries is exact here)
        if (rc != MBPE_OK) return rc;
        if (c->opt_time_kernels) {
            rc = ensure_events(c->kev, 2ull * batch);
            if (rc != MBPE_OK) return rc;
        }
        rc = timed_group(c, [&]() -> int {
            for (uint32_t i = 0; i < batch; ++i) {
                step_local(c, c->opt_time_kernels ? (int)i : -1);
                const int r = finish_unit(c, Phase::StepDeltas);
                if (r != MBPE_OK) return r;
                c->k++;
            }
            return MBPE_OK;
        });
        if (rc != MBPE_OK) return rc;
        if (c->opt_time_kernels) {
            for (uint32_t i = 0; i < batch; ++i) {
                float km = 0;
                HIPCHK(hipEventElapsedTime(&km, c->kev[2 * i], c->kev[2 * i + 1]));
                c->stats.ms_merge_kernel += km;
                c->stats.merge_launches++;
            }
        }
        {
            // Did the table run out of pairs with a count?  best[k - batch .. k] are the pairs of this batch's steps and
            // of the next one.  Merging a pair that occurs nowhere changes neither the stream nor the table, so every
            // later choice is that pair again: `first` ends there like the reference's loop (its rebuilt table is empty,
            // Tokenizer.h:586-588), `lexical` keeps choosing it: the rest of this call's steps are filled in (fill_zero_tail).
            std::vector<unsigned long long> hb(batch + 1);
            HIPCHK(hipMemcpy(hb.data(), c->best + (c->k - batch), hb.size() * 8, hipMemcpyDeviceToHost));
            uint32_t z = 0;
            while (z <= batch && (hb[z] >> 32) != 0) ++z;
            if (z <= batch) {
                const uint32_t kz = c->k - batch + z;          // the first step whose pair has count 0
                if (c->opt_first) {
                    done += z;
                    c->k = kz;
                    c->n_target = kz;
                } else {
                    const uint32_t target = std::min<uint64_t>((uint64_t)c->k + (n_steps - done - batch), c->n_target);
                    done += batch + (target - c->k);
                    rc = fill_zero_tail(c, hb[z], c->k + 1, target, false);      // (best[k] is that pair already)
                    if (rc != MBPE_OK) return rc;
                }
                rc = after_batch(c);
                if (rc != MBPE_OK) return rc;
                break;
            }
        }
        done += batch;
        rc = after_batch(c);
        if (rc != MBPE_OK) return rc;
    }
    if (steps_done_out) *steps_done_out = done;
    return MBPE_OK;
}

// slot stream + hashed pair table of the 16-bit part -> the 32-bit loop (WideRun::convert).  From here on the training's
// stream, table and merge counter live in c->wr; the 16-bit buffers go back to the pool (their merges stay in best[]).
static int wide_convert(mbpe_ctx *c) {
    int rc = sync_ctl(c);
    if (rc != MBPE_OK) return rc;
    rc = do_compact(c);                       // no holes left: the first n_live slots are the stream (barriers included)
    if (rc != MBPE_OK) return rc;
    const WideSlots src = {c->tok[c->cur], c->h_ctl.n_live, c->barrier ? c->n_barriers : 0,
                           c->barrier ? kBarrier : 0xFFFFFFFFu, c->chunked && !c->barrier ? kEndBit : 0u,
                           c->tab.ekey, c->tab.ecnt, c->h_ctl.n_entries, c->last_top};
    rc = c->wr.convert(wide_dev(c), src, WideGoal{c->n_target_total - c->n_target, 256 + c->n_target, c->opt_first != 0});
    if (rc != MBPE_OK) return rc;
    free_slot_stream(c);
    c->pool.trim();
    return MBPE_OK;
}

// `first` mode: did the slot stream's share already end where the reference's loop breaks (no pair left,
// Tokenizer.h:586-588)?  Then there is nothing to continue: the result is the merges so far, as at a smaller vocabulary.
static int first_ran_out(mbpe_ctx *c, bool *out) {
    *out = false;
    if (!c->opt_first) return MBPE_OK;
    if (c->n_target < c->vocab_size - 256) { *out = true; return MBPE_OK; }     // (the one-merge loop cut n_target there)
    if (c->k == 0) return MBPE_OK;
    unsigned long long last = 0;
    HIPCHK(hipMemcpy(&last, c->best + (c->k - 1), 8, hipMemcpyDeviceToHost));
    *out = (last >> 32) == 0;
    return MBPE_OK;
}

int mbpe_train_steps(mbpe_ctx *c, uint32_t n_steps, uint32_t *steps_done_out) {
    if (steps_done_out) *steps_done_out = 0;
    if (!c) return MBPE_ERR_ARG;
    if (!c->begun) { mbpe_host::set_last_error("mbpe_train_steps before mbpe_train_begin"); return MBPE_ERR_STATE; }
    if (c->pending != Phase::None) { mbpe_host::set_last_error("an exchange is pending: call mbpe_comm_exchange_done"); return MBPE_ERR_STATE; }
    HIPCHK(hipSetDevice(c->device));
    if (!c->wide) return train_steps16(c, n_steps, steps_done_out);
    // a training that continues on 32-bit tokens: the slot stream's share first, then the conversion, then the rest
    uint32_t done = 0;
    if (!c->wr.active) {
        int rc = train_steps16(c, n_steps, &done);
        if (steps_done_out) *steps_done_out = done;
        if (rc != MBPE_OK || done >= n_steps || c->exhausted || c->k < c->n_target) return rc;
        bool out = false;
        rc = first_ran_out(c, &out);
        if (rc != MBPE_OK || out) return rc;
        rc = wide_convert(c);
        if (rc != MBPE_OK) return rc;
    }
    uint32_t more = 0;
    int rc = c->wr.steps(wide_dev(c), n_steps - done, &more);
    if (steps_done_out) *steps_done_out = done + more;
    return rc;
}

int mbpe_train_sequences(mbpe_ctx *c, uint32_t n_sequences, uint32_t *merges_done_out) {
    if (merges_done_out) *merges_done_out = 0;
    if (!c) return MBPE_ERR_ARG;
    if (!c->begun) { mbpe_host::set_last_error("mbpe_train_sequences before mbpe_train_begin"); return MBPE_ERR_STATE; }
    if (c->pending != Phase::None || (is_multi(c) && c->comm_external)) {
        mbpe_host::set_last_error("mbpe_train_sequences: not available with an external transport (use mbpe_train_steps)");
        return MBPE_ERR_STATE;
    }
    if (c->wr.active || (c->wide && c->k >= c->n_target))
        return mbpe_train_steps(c, n_sequences, merges_done_out);                    // (32-bit loop: one merge per pass)
    if (!use_batches(c)) return mbpe_train_steps(c, n_sequences, merges_done_out);   // one merge per pass
    HIPCHK(hipSetDevice(c->device));
    return train_steps_batched(c, c->n_target, merges_done_out, n_sequences);
}

int mbpe_comm_exchange_buffer(mbpe_ctx *c, void **dev_ptr_out, uint64_t *n_u32_out) {
    if (!c || !dev_ptr_out || !n_u32_out) return MBPE_ERR_ARG;
    if (c->pending == Phase::None) { mbpe_host::set_last_error("no exchange pending"); return MBPE_ERR_STATE; }
    *dev_ptr_out = c->pending_x.buf;
    *n_u32_out = c->pending_x.words;
    return MBPE_OK;
}

// External transport: the caller has made the pending exchange.  Continues the unit behind it; when the whole unit is on
// the stream, ends it as the loops of one rank do and starts the next one while the call's target is not reached.
int mbpe_comm_exchange_done(mbpe_ctx *c) {
    if (!c) return MBPE_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    const Phase p = c->pending;
    if (p == Phase::None) { mbpe_host::set_last_error("no exchange pending"); return MBPE_ERR_STATE; }
    c->pending = Phase::None;
    const Phase next = continue_after(c, p);
    if (next != Phase::None) return suspend(c, next);
    if (p == Phase::BeginCounts || p == Phase::BeginFirst) return begin_end(c);
    const bool batched = p == Phase::SeqEdges;      // a batch sequence; otherwise a one-merge step
    if (!batched) c->k++;
    int rc = sync_ctl(c);
    if (rc != MBPE_OK) return rc;
    HIPCHK(hipGetLastError());
    const uint32_t before = c->k;
    if (batched) c->k = c->h_ctl.k_done;
    rc = after_batch(c);
    if (rc != MBPE_OK) return rc;
    if (c->k >= c->pending_target || (batched && c->k == before)) return MBPE_OK;      // (a sequence that merged nothing: none left)
    return start_unit_external(c, batched);
}

int mbpe_train_result(mbpe_ctx *c, uint32_t *merges_out, int32_t *counts_out, uint32_t cap_merges,
                      uint32_t *n_merges_out) {
    if (!c) return MBPE_ERR_ARG;
    if (!c->begun) { mbpe_host::set_last_error("mbpe_train_result before mbpe_train_begin"); return MBPE_ERR_STATE; }
    HIPCHK(hipSetDevice(c->device));
    uint32_t n = c->exhausted ? c->n_prior : c->n_valid;
    std::vector<unsigned long long> h(n);
    if (n && !c->wide_direct) HIPCHK(hipMemcpy(h.data(), c->best, (size_t)n * 8, hipMemcpyDeviceToHost));
    if (c->opt_first && !c->wide_direct) {
        // a table rebuilt before every merge holds no zero-count pair: the reference's loop breaks as soon as
        // no pair is left (Tokenizer.h:586-588), the incremental table only shows it as "max count 0"
        uint32_t real = 0;
        while (real < n && (h[real] >> 32) != 0) ++real;
        n = real;
    }
    const uint32_t nw = c->wr.n_merges();      // merges of the 32-bit continuation
    if (n_merges_out) *n_merges_out = n + nw;
    if (n + nw > cap_merges && merges_out) { mbpe_host::set_last_error("merges_out too small"); return MBPE_ERR_ARG; }
    if (!(n + nw) || !merges_out) return MBPE_OK;
    for (uint32_t i = 0; i < n && c->wide_direct; ++i) {      // (all of them prior merges, kept as they were given)
        merges_out[2 * i] = c->h_prior_raw[2 * i];
        merges_out[2 * i + 1] = c->h_prior_raw[2 * i + 1];
        if (counts_out) counts_out[i] = -1;
    }
    for (uint32_t i = 0; i < n && !c->wide_direct; ++i) {
        uint32_t key = ~(uint32_t)h[i];
        merges_out[2 * i] = key >> 16;
        merges_out[2 * i + 1] = key & 0xFFFFu;
        if (counts_out) counts_out[i] = (int32_t)(h[i] >> 32);
    }
    c->wr.merges(merges_out + 2 * (size_t)n, counts_out ? counts_out + n : nullptr);
    return MBPE_OK;
}

int mbpe_get_stats(mbpe_ctx *c, mbpe_stats *out) {
    if (!c || !out) return MBPE_ERR_ARG;
    c->stats.n_slots = c->begun ? c->n_slots : 0;
    c->stats.n_live = c->begun ? c->h_ctl.n_live - (c->barrier ? c->n_barriers : 0) : 0;      // (barriers are no tokens)
    c->stats.n_merges = c->exhausted ? c->n_prior : c->n_valid;
    c->stats.n_pairs = c->begun ? c->h_ctl.n_entries : 0;
    c->stats.n_batches = c->begun ? (use_batches(c) ? c->h_ctl.n_batches : c->k - c->n_prior) : 0;
    c->stats.n_fused = c->begun ? c->h_ctl.n_fused : 0;
    c->stats.n_fused_dropped = c->begun ? c->h_ctl.n_fused_dropped : 0;
    c->stats.cut_conflict = c->begun ? c->h_ctl.cut_conflict : 0;
    c->stats.cut_bucket = c->begun ? c->h_ctl.cut_bucket : 0;
    c->stats.cut_single = c->begun ? c->h_ctl.cut_single : 0;
    c->stats.cut_full = c->begun ? c->h_ctl.cut_full : 0;
    c->stats.n_validation_drops = c->begun ? c->h_ctl.n_validation_drops : 0;
    c->stats.n_sel_fallback = c->begun ? c->h_ctl.n_sel_fallback : 0;
    c->stats.log_spilled = c->begun ? c->h_ctl.log_spilled : 0;
    c->stats.log_passes = c->begun ? c->h_ctl.log_passes : 0;
    c->stats.log_refills = c->begun ? c->h_ctl.log_refills : 0;
    c->stats.n_sel_retry = c->begun ? c->h_ctl.n_sel_retry : 0;
    c->stats.adapt_limit = c->begun ? c->h_ctl.adapt_limit : 0;
    c->stats.n_sel_blocks = c->begun ? c->h_ctl.n_sel_blocks : 0;
    for (int i = 0; i < 8; ++i) c->stats.size_hist[i] = c->begun ? c->h_ctl.size_hist[i] : 0;
    c->stats.n_skipped = c->begun ? c->h_ctl.n_skipped : 0;
    c->stats.n_skip_cut = c->begun ? c->h_ctl.n_skip_cut : 0;
    if (c->begun && c->wr.active) c->wr.add_stats(&c->stats);
    *out = c->stats;
    return MBPE_OK;
}

int mbpe_train(mbpe_ctx *c, const uint8_t *text, uint64_t n_bytes, const uint64_t *chunk_off, uint64_t n_chunks,
               uint32_t vocab_size, int conflict_resolution, uint32_t *merges_out, int32_t *counts_out,
               uint32_t *n_merges_out, mbpe_stats *stats_out) {
    return mbpe_train_from(c, text, n_bytes, chunk_off, n_chunks, vocab_size, conflict_resolution, nullptr, 0, merges_out,
                           counts_out, n_merges_out, stats_out);
}

int mbpe_train_from(mbpe_ctx *c, const uint8_t *text, uint64_t n_bytes, const uint64_t *chunk_off, uint64_t n_chunks,
                    uint32_t vocab_size, int conflict_resolution, const uint32_t *prior_merges, uint32_t n_prior,
                    uint32_t *merges_out, int32_t *counts_out, uint32_t *n_merges_out, mbpe_stats *stats_out) {
    if (!c || !merges_out) { mbpe_host::set_last_error("mbpe_train: NULL argument"); return MBPE_ERR_ARG; }
    if (conflict_resolution != 0 && conflict_resolution != 1) {
        mbpe_host::set_last_error("conflict_resolution: 0 = first, 1 = lexical");
        return MBPE_ERR_ARG;
    }
    int rc = mbpe_load_corpus(c, text, n_bytes, chunk_off, n_chunks, 0);
    if (rc != MBPE_OK) return rc;
    const int64_t keep = c->opt_first;
    c->opt_first = conflict_resolution == 0;
    rc = mbpe_train_begin_from(c, vocab_size, prior_merges, n_prior);
    if (rc == MBPE_OK) rc = mbpe_train_steps(c, vocab_size - 256, nullptr);
    if (rc == MBPE_OK) rc = mbpe_train_result(c, merges_out, counts_out, vocab_size - 256, n_merges_out);
    if (rc == MBPE_OK && stats_out) mbpe_get_stats(c, stats_out);
    c->opt_first = keep;
    return rc;
}

int mbpe_train_lexical(mbpe_ctx *c, const uint8_t *text, uint64_t n_bytes, const uint64_t *chunk_off,
                       uint64_t n_chunks, uint32_t vocab_size, uint32_t *merges_out, int32_t *counts_out,
                       uint32_t *n_merges_out, mbpe_stats *stats_out) {
    return mbpe_train(c, text, n_bytes, chunk_off, n_chunks, vocab_size, 1, merges_out, counts_out, n_merges_out,
                      stats_out);
}

int mbpe_get_stream(mbpe_ctx *c, uint32_t *tokens_out, uint8_t *chunk_end_out, uint64_t cap, uint64_t *n_out) {
    if (!c || !n_out) return MBPE_ERR_ARG;
    if (!c->begun) { mbpe_host::set_last_error("mbpe_get_stream before mbpe_train_begin"); return MBPE_ERR_STATE; }
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (c->wr.active) return c->wr.get_stream(c->chunked, tokens_out, chunk_end_out, cap, n_out);
    std::vector<uint16_t> h(c->n_slots);
    HIPCHK(hipMemcpy(h.data(), c->tok[c->cur], c->n_slots * 2, hipMemcpyDeviceToHost));
    const bool endflag = c->chunked && !c->barrier;
    const uint32_t idmask = endflag ? 0x7FFFu : 0xFFFFu;
    uint64_t w = 0;
    for (uint64_t i = 0; i < c->n_slots; ++i) {
        if (h[i] == kHole) continue;
        if (c->barrier && h[i] == kBarrier) {          // ends the chunk of the token before it
            if (tokens_out && chunk_end_out && w) chunk_end_out[w - 1] = 1;
            continue;
        }
        if (tokens_out) {
            if (w >= cap) { mbpe_host::set_last_error("tokens_out too small"); return MBPE_ERR_ARG; }
            tokens_out[w] = h[i] & idmask;
            if (chunk_end_out) chunk_end_out[w] = endflag ? (h[i] >> 15) & 1 : 0;
        }
        ++w;
    }
    *n_out = w;
    return MBPE_OK;
}

int mbpe_stream_device(mbpe_ctx *c, const void **slots_out, uint64_t *n_slots_out, uint32_t *slot_bits_out,
                       uint32_t *end_bit_out, uint32_t *barrier_out) {
    if (!c || !slots_out || !n_slots_out) return MBPE_ERR_ARG;
    if (!c->begun) { mbpe_host::set_last_error("mbpe_stream_device before mbpe_train_begin"); return MBPE_ERR_STATE; }
    HIPCHK(hipSetDevice(c->device));
    if (c->wr.active) return c->wr.stream_device(wide_dev(c), slots_out, n_slots_out, slot_bits_out, end_bit_out, barrier_out);
    int rc = sync_ctl(c);          // also refreshes which of the two buffers is live
    if (rc != MBPE_OK) return rc;
    *slots_out = c->tok[c->cur];
    *n_slots_out = c->n_slots;
    if (slot_bits_out) *slot_bits_out = 16;
    if (end_bit_out) *end_bit_out = c->chunked && !c->barrier ? kEndBit : 0;
    if (barrier_out) *barrier_out = c->barrier ? kBarrier : MBPE_NO_BARRIER;
    return MBPE_OK;
}

int mbpe_table_device(mbpe_ctx *c, const void **cells_out, uint32_t *vshift_out) {
    if (!c || !cells_out || !vshift_out) return MBPE_ERR_ARG;
    if (!c->begun) { mbpe_host::set_last_error("mbpe_table_device before mbpe_train_begin"); return MBPE_ERR_STATE; }
    HIPCHK(hipSetDevice(c->device));
    if (c->wr.active) { mbpe_host::set_last_error("the pair table is hashed (no dense view)"); return MBPE_ERR_STATE; }
    int rc = sync_ctl(c);
    if (rc != MBPE_OK) return rc;
    if (!c->tab.cells) { mbpe_host::set_last_error("the pair table is hashed (no dense view)"); return MBPE_ERR_STATE; }
    *cells_out = c->tab.cells;
    *vshift_out = c->tab.vshift;
    return MBPE_OK;
}

int mbpe_get_pairs(mbpe_ctx *c, uint32_t *first_out, uint32_t *second_out, int32_t *count_out, uint64_t cap,
                   uint64_t *n_out) {
    if (!c || !n_out) return MBPE_ERR_ARG;
    if (!c->begun) { mbpe_host::set_last_error("mbpe_get_pairs before mbpe_train_begin"); return MBPE_ERR_STATE; }
    HIPCHK(hipSetDevice(c->device));
    if (c->wr.active) return c->wr.get_pairs(wide_dev(c), first_out, second_out, count_out, cap, n_out);
    int rc = sync_ctl(c);
    if (rc != MBPE_OK) return rc;
    const uint64_t n = c->h_ctl.n_entries;
    *n_out = n;
    if (!first_out) return MBPE_OK;
    if (cap < n) { mbpe_host::set_last_error("pair arrays too small"); return MBPE_ERR_ARG; }
    if (c->tab.cells) {
        // dense layout: 32 x 32 tiles, row-major; copy the tile rows that hold ids that exist
        const uint32_t pitch = 1u << c->tab.vshift, ids = std::min<uint32_t>(256 + c->k, pitch);
        const uint32_t tpr = pitch / 32, used_tiles = (ids + 31) / 32;
        std::vector<uint32_t> rowbuf((size_t)used_tiles * 1024);
        struct Rec { uint32_t f, s; int32_t c; };
        std::vector<Rec> recs;
        recs.reserve(n);
        for (uint32_t tr = 0; tr < used_tiles; ++tr) {
            HIPCHK(hipMemcpy(rowbuf.data(), c->tab.cells + (size_t)tr * tpr * 1024, rowbuf.size() * 4,
                             hipMemcpyDeviceToHost));
            for (uint32_t fr = 0; fr < 32; ++fr)
                for (uint32_t tc = 0; tc < used_tiles; ++tc)
                    for (uint32_t sc = 0; sc < 32; ++sc) {
                        const uint32_t v = rowbuf[(size_t)tc * 1024 + fr * 32 + sc];
                        if (v & kPresent) recs.push_back({tr * 32 + fr, tc * 32 + sc, (int32_t)(v & ~kPresent)});
                    }
        }
        uint64_t o = recs.size();
        if (o > n) { mbpe_host::set_last_error("pair table holds more pairs than counted"); return MBPE_ERR_OVERFLOW; }
        for (uint64_t i = 0; i < o; ++i) {
            first_out[i] = recs[i].f;
            second_out[i] = recs[i].s;
            if (count_out) count_out[i] = recs[i].c;
        }
        if (o != n) { mbpe_host::set_last_error("pair table holds fewer pairs than counted"); return MBPE_ERR_OVERFLOW; }
        return MBPE_OK;
    }
    std::vector<uint32_t> keys(n);
    std::vector<int32_t> cnts(n);
    if (n) {
        HIPCHK(hipMemcpy(keys.data(), c->tab.ekey, n * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(cnts.data(), c->tab.ecnt, n * 4, hipMemcpyDeviceToHost));
    }
    for (uint64_t i = 0; i < n; ++i) {
        first_out[i] = keys[i] >> 16;
        second_out[i] = keys[i] & 0xFFFFu;
        if (count_out) count_out[i] = cnts[i];
    }
    return MBPE_OK;
}

int mbpe_compact(mbpe_ctx *c) {
    if (!c) return MBPE_ERR_ARG;
    if (!c->begun) { mbpe_host::set_last_error("mbpe_compact before mbpe_train_begin"); return MBPE_ERR_STATE; }
    HIPCHK(hipSetDevice(c->device));
    if (c->wr.active) return MBPE_OK;        // (the 32-bit stream has no holes)
    int rc = sync_ctl(c);
    if (rc != MBPE_OK) return rc;
    return do_compact(c);
}

// ---- multi-GPU transport ------------------------------------------------------

static int comm_allreduce(mbpe_ctx *c, uint32_t *buf, size_t count) {
    Rccl &r = rccl();
    if (!r.ok || !c->nccl_comm) { mbpe_host::set_last_error("RCCL communicator not initialised"); return MBPE_ERR_COMM; }
    int rc = r.AllReduce(buf, buf, count, (int)ncclUint32, (int)ncclSum, c->nccl_comm, c->stream);
    if (rc != 0) {
        mbpe_host::set_last_error(std::string("ncclAllReduce: ") + r.GetErrorString(rc));
        return MBPE_ERR_COMM;
    }
    return MBPE_OK;
}

int mbpe_comm_unique_id(uint8_t *id_out) {
    if (!id_out) return MBPE_ERR_ARG;
    Rccl &r = rccl();
    if (!r.ok) { mbpe_host::set_last_error(r.why); return MBPE_ERR_COMM; }
    static_assert(sizeof(ncclUniqueId) == MBPE_COMM_ID_BYTES, "unique id size");
    ncclUniqueId id;
    int rc = r.GetUniqueId(&id);
    if (rc != 0) { mbpe_host::set_last_error(std::string("ncclGetUniqueId: ") + r.GetErrorString(rc)); return MBPE_ERR_COMM; }
    memcpy(id_out, &id, sizeof(id));
    return MBPE_OK;
}

int mbpe_comm_init(mbpe_ctx *c, const uint8_t *id, int rank, int n_ranks) {
    if (!c || !id || n_ranks < 1 || rank < 0 || rank >= n_ranks) {
        mbpe_host::set_last_error("mbpe_comm_init: bad argument");
        return MBPE_ERR_ARG;
    }
    if (c->begun || c->pending != Phase::None) { mbpe_host::set_last_error("mbpe_comm_init after mbpe_train_begin"); return MBPE_ERR_STATE; }
    HIPCHK(hipSetDevice(c->device));
    Rccl &r = rccl();
    if (!r.ok) { mbpe_host::set_last_error(r.why); return MBPE_ERR_COMM; }
    if (c->nccl_comm) { r.CommDestroy(c->nccl_comm); c->nccl_comm = nullptr; }
    ncclUniqueId uid;
    memcpy(&uid, id, sizeof(uid));
    int rc = r.CommInitRank(&c->nccl_comm, n_ranks, uid, rank);
    if (rc != 0) {
        mbpe_host::set_last_error(std::string("ncclCommInitRank: ") + r.GetErrorString(rc));
        c->nccl_comm = nullptr;
        return MBPE_ERR_COMM;
    }
    c->rank = rank;
    c->n_ranks = n_ranks;
    c->comm_external = false;
    return MBPE_OK;
}

int mbpe_comm_init_external(mbpe_ctx *c, int rank, int n_ranks) {
    if (!c || n_ranks < 1 || rank < 0 || rank >= n_ranks) {
        mbpe_host::set_last_error("mbpe_comm_init_external: bad argument");
        return MBPE_ERR_ARG;
    }
    if (c->begun || c->pending != Phase::None) { mbpe_host::set_last_error("mbpe_comm_init_external after mbpe_train_begin"); return MBPE_ERR_STATE; }
    c->rank = rank;
    c->n_ranks = n_ranks;
    c->comm_external = true;
    return MBPE_OK;
}

}  // extern "C"
