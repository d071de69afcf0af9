// Device-side data layout shared by the HIP kernels (kernels.hip) and the
// host orchestration (train.cpp).  See DESIGN.md "Data layout in HBM".
#ifndef MBPE_DEV_H
#define MBPE_DEV_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mbpe {

// ---- token stream -----------------------------------------------------
// The corpus is a stream of 16-bit SLOTS.  A slot is either a live token or
// a HOLE left behind by a merge (the second token of a merged pair); holes
// are squeezed out by an occasional compaction pass.  In a chunked corpus
// bit 15 of a live slot marks "last token of its chunk" (no pair starts at
// such a token: Tokenizer.h:135-144, :311-319).
constexpr uint32_t kHole = 0xFFFFu;    // also "no token" in tile summaries
constexpr uint32_t kEndBit = 0x8000u;  // chunked corpora only
// A chunked corpus whose ids do not fit 15 bits keeps the chunk ends as BARRIER slots instead: a live token
// (kBarrier, an id no token has: below the stand-in ids of kTTMax (t,t) members, see MBPE_TT_MAX) after the last
// token of every chunk.  It belongs to no pair and is never merged; ids then use all 16 bits.
constexpr uint32_t kBarrier = 0xFFEEu;

constexpr int kTile = 512;             // slots per tile = one wave x 8 slots (one 16-byte load per lane)
constexpr int kMergeThreads = 256;     // 4 waves per workgroup, each wave walks its own tiles
// the kernels that hold the batch lookup table in LDS: one table per workgroup, so a large table
// wants a large workgroup (4 waves per SIMD either way)
#ifndef MBPE_LUT_THREADS
#define MBPE_LUT_THREADS 1024
#endif
constexpr int kLutThreads = MBPE_LUT_THREADS;
constexpr int kSlotsPerLane = 8;

// What a tile exposes to its neighbours.  A merge pass reads these (never the
// neighbour's slots) and leaves them untouched; the new summaries of changed
// tiles are staged in a side array and folded in after the pass, so in-place
// rewriting cannot race with halo reads.
struct __attribute__((aligned(16))) TileSum {
    uint16_t head0, head1;   // first / second live token (kHole if absent)
    uint16_t tail1, tail0;   // second-last / last live token
    uint16_t n_live;         // live tokens in the tile
    uint16_t tail_run;       // trailing live tokens equal (raw) to tail0
    uint16_t pad0, pad1;
};
static_assert(sizeof(TileSum) == 16, "TileSum must be 16 bytes");

// What a rank exposes to its neighbours in a multi-GPU run: the same
// information for the whole shard (looked through empty tiles).
struct RankEdge {
    uint32_t head0, head1;   // first two live tokens of the shard
    uint32_t tail1, tail0;   // last two live tokens of the shard
    uint32_t n_live_lo, n_live_hi;
    uint32_t tail_run_lo, tail_run_hi;  // trailing run of tail0 (raw)
};

// ---- pair table ---------------------------------------------------------
// Open-addressing hash (key -> entry index; key and index share one 8-byte slot, so
// a probe is one memory access) plus dense entry arrays that the
// argmax kernel scans.  key = (first << 16) | second.  Entries are never
// removed: PairCountLexicalOrder never erases (PairCount.h:249-260), so a
// pair whose count returned to 0 is still a candidate (SURVEY.md 8-S rule 4).
constexpr uint32_t kEmptyKey = 0xFFFFFFFFu;
constexpr unsigned long long kEmptySlot = 0xFFFFFFFFFFFFFFFFull;

constexpr int kBlockShift = 10;                 // argmax hierarchy: 1024 entries per block,
constexpr uint32_t kBlockSize = 1u << kBlockShift;   // 1024 blocks per super-block

// Pair table, two layouts behind the same device functions (table_add, entry_packed):
//  * dense (cells != NULL; vocab <= 32,768): one u32 per possible pair, stored as tiles of
//    32 x 32 (first, second) cells (see dense_index in kernels.hip), value = kPresent | count
//    for a pair that was ever inserted, 0 otherwise.  No hashing, no growth; inserts of a new
//    token's pairs and updates along a row come in contiguous runs.  ecap = number of cells
//    = 1 << (2 * vshift), vshift = log2 of the vocabulary rounded up to a power of two (>= 256).
//  * hashed (larger vocabularies): open addressing over appended entries.
// "Entry index" below means the cell index (dense) or the append index (hashed).
struct PairTable {
    unsigned long long *hslot;   // [hcap] (key << 32) | entry index; kEmptySlot when free
    uint32_t *ekey;      // [ecap]
    int32_t  *ecnt;      // [ecap]
    unsigned long long *bmax;   // [ecap / 1024 + 1] upper bound of packed (count, ~key) per block
    unsigned long long *smax;   // [ecap / 1024^2 + 1] upper bound per super-block
    uint32_t  hmask;     // hcap - 1
    uint32_t  ecap;
    uint32_t *cells;     // dense layout, else NULL
    uint32_t  vshift;    // log2 of the row pitch of the dense layout
};
constexpr uint32_t kPresent = 0x80000000u;

// Mutable scalars shared by the kernels of one context.
struct DevCtl {
    uint32_t n_entries;      // pairs ever inserted (== PairCount::get_count())
    uint32_t err;            // sticky error bits, see kErr*
    uint32_t m;              // matches of the current merge (this rank)
    uint32_t adj;            // adjacent match pairs of the current merge
    unsigned long long removed_total;  // holes created since the last compaction
    unsigned long long n_live;         // live tokens in this rank's shard
    unsigned long long scan_total;     // output of the tile scan (compaction)
    uint32_t rm;             // tokens removed from THIS rank's shard by the current merge
    // ---- batched merges: the merge counter lives on the device ----
    uint32_t k_done;         // merges committed so far
    uint32_t k_limit;        // do not go beyond this many merges (host sets it per call)
    uint32_t batch_n;        // candidates selected for the current batch (0: nothing to do)
    uint32_t commit_n;       // how many of them survive validation
    uint32_t n_batches;      // batches that did work (statistics)
    uint32_t n_marked;       // tiles in the rewrite list of the current batch
    uint32_t cur;            // which of the two token buffers holds the stream (batch sequences)
    uint32_t fused;          // the current batch is large enough for the fused pass (k_fused_batch)
    uint32_t n_fused;        // fused passes run / of them abandoned by validation (statistics)
    uint32_t n_fused_dropped;
    uint32_t cut_conflict, cut_bucket, cut_single, cut_full;   // why batches ended (statistics)
    uint32_t n_validation_drops;
    // ---- threshold selection (k_sel_scan / k_sel_pick) ----
    unsigned long long sel_T;   // gather every entry with packed value >= sel_T (0: not primed)
    uint32_t sel_n;             // entries gathered by the current scan
    uint32_t sel_ok;            // the current batch was selected from the gathered list
    uint32_t n_sel_fallback;    // batches selected by the bound-walking kernel instead (statistics)
    uint32_t sel_retry;         // the first gather overflowed: a second one with a higher threshold follows
    uint32_t adapt_limit;       // batch size limit learnt from validation (0: none yet = kBatchMax)
    uint32_t recent_n;          // running mean of the batch sizes (k_sel_pick: how far the next candidate list should reach)
    uint32_t n_sel_retry;       // statistics
    uint32_t sel_mode;          // 1: the next first gather lists block bounds (to find a threshold), not entries
    uint32_t n_ranks;           // shards of the stream (1 without multi-GPU); set at begin
    uint32_t size_hist[8];      // committed batch sizes: 1, 2-3, 4-7, ..., 128+ (statistics)
    uint32_t n_skipped;         // dependent candidates passed over / batches cut short because one of them
    uint32_t n_skip_cut;        //   had not fallen behind after all (statistics)
    uint32_t skip_off;          // batches during which dependent candidates end the batch again (after a failed pass-over)
    uint32_t skip_penalty;      // length of the next such period (doubles on failure, halves on success)
    uint32_t skip_failed;       // set by k_validate for k_seq_finish
    uint32_t skip_red_q16;      // what passed-over candidates lost lately, as a fraction of their count (low estimate)
    unsigned long long n_sel_blocks;   // blocks read by the gathers (statistics)
    // ---- `first` tie-break inside batch sequences ----
    uint32_t first_mode;        // (host, at begin) ties between equal counts are decided by stream position, not by key:
                                //   a batch only takes pairs whose counts differ from every other candidate's, and
                                //   validation treats an equal count like a larger one
    uint32_t first_tie;         // the selection took ONE pair whose count is shared: k_first_* pick the one that comes first
    uint32_t marks_all;         // the fused pass of this sequence wrote EVERY tile's summary to the side array and set no
                                //   tile marks (its tiles nearly all change): "every tile is marked"
    uint32_t cells_on;          // (host sets 1 at begin when the delta log exists) matches between two raw bytes are
                                //   logged as records and counted behind the pass (k_log_count); k_seq_finish clears it for
                                //   good once fewer than half of a large batch's matches were of that kind
    uint32_t cell_hits;         // matches of that kind in the sequence under way (k_log_count; the pass itself adds those
                                //   that found the log full)
    uint32_t cells_min;         // (host, at begin) batches of at least this many pairs log (kCellsMinBatch; 2 when the
                                //   "pair_cells" option forces the log on: tests)
    uint32_t adj_pitch;         // (host, at begin) row pitch of the ADJ block: the largest batch this training can select
                                //   ("max_batch" rounded up to 64), so that the block -- and what several GPUs exchange of
                                //   it -- is as small as the batches allow
    uint32_t log_spilled;       // eligible matches that found the log full and took the two L / R atomics (statistics)
    uint32_t log_passes;        // passes whose log held records (statistics)
    uint32_t log_refills;       // chunks taken by waves that had used one up before (statistics)
    uint32_t log_refused;       // (k_log_plan) the pass under way would have logged, but its pairs' counts exceed the
                                //   partition buffer: it says nothing about the share of byte neighbours (k_seq_finish)

};

// A batch holds up to kBatchMax pairs that can be merged in ONE pass over the
// stream (see k_select_batch).  Per batch scratch, device memory:
#ifndef MBPE_BATCH_MAX
#define MBPE_BATCH_MAX 4096
#endif
constexpr int kBatchMax = MBPE_BATCH_MAX;
// ("max_batch" when the caller sets none.  2048 while the candidate window was sized by the batch limit alone -- at 4096
//  of the 8192 list entries every other gather overflowed or ran short; since the window follows the batch sizes the
//  full cap is the fastest: 66 passes against 70 on the benchmark)
constexpr int kBatchDefault = kBatchMax;
static_assert((kBatchMax & (kBatchMax - 1)) == 0 && kBatchMax >= 64,
              "a power of two: grid strides over the delta arrays keep a thread on one pair index");
// candidates gathered by k_sel_scan
#ifndef MBPE_SEL_CAP
#define MBPE_SEL_CAP 8192
#endif
constexpr uint32_t kSelCap = MBPE_SEL_CAP;
struct SelList {
    unsigned long long packed[kSelCap];
    uint32_t eidx[kSelCap];
};

// (t,t) members of a batch: each needs an id no token has (idmask - 1 - i) and a slot of its own in the
// kernels' token -> id map
#ifndef MBPE_TT_MAX
#define MBPE_TT_MAX 16
#endif
constexpr int kTTMax = MBPE_TT_MAX;
static_assert(0xFFFFu - (uint32_t)MBPE_TT_MAX > kBarrier, "the barrier id must lie below the stand-in ids");
constexpr uint32_t kTTSlots = 256;
#ifndef MBPE_SKIP_MAX
#define MBPE_SKIP_MAX 32
#endif
constexpr int kSkipMax = MBPE_SKIP_MAX;
// batches of at least this many pairs log their matches between raw bytes (smaller ones are not bound by their atomics:
// there the extra tests cost more than the saved atomics)
constexpr uint32_t kCellsMinBatch = 512;

// The delta log (kernels.hip, "the delta log").  A record is (j << 16) | (x << 8) | y: one match of batch pair j between
// the raw bytes x and y.  Buckets are 64 consecutive pairs: 64 x (256 L + 256 R) counters fill the LDS of k_log_count.
constexpr uint32_t kLogNull = 0xFFFFFFFFu;          // no record (the unused tail of a chunk)
constexpr uint32_t kLogBucketPairs = 64;
constexpr uint32_t kLogBuckets = (uint32_t)MBPE_BATCH_MAX / kLogBucketPairs;
constexpr uint32_t kLogChunkMin = 256;              // records: a tile's most, so a wave's chunk always holds the next tile
constexpr uint32_t kLogChunkDefault = 4096;
static_assert(MBPE_BATCH_MAX % 64 == 0 && MBPE_BATCH_MAX <= 65536, "a record holds the pair index in 16 bits");
struct LogState {
    uint32_t cap;               // (host, at begin) records the log holds: a multiple of `chunk`
    uint32_t chunk;             // (host, at begin) records a wave reserves at a time: a multiple of kLogChunkMin
    uint32_t part_cap;          // (host, at begin) records the partition buffer holds
    uint32_t on;                // (k_log_plan) this pass logs
    uint32_t cursor;            // next free record of the log: waves add `chunk` (may run past cap: refused)
    uint32_t n_buckets;
    uint32_t base[kLogBuckets + 1];     // region of every bucket in the partition buffer: prefix sums of the pairs' counts
    uint32_t fill[kLogBuckets];         // records placed there so far
};
constexpr uint32_t kNoTT = 0xFFFFFFFFu;
struct BatchState {
    uint32_t key[kBatchMax];      // (first << 16) | second
    uint32_t eidx[kBatchMax];     // entry index in the pair table
    unsigned long long packed[kBatchMax];   // (count << 32) | ~key, as in best[]
    unsigned long long maxp[kBatchMax];     // largest packed (count, ~key) of the pairs merge j creates (k_delta_max)
    uint32_t adj_in[kBatchMax];   // sum_p ADJ[p][j]: matches of j directly after another match of the batch
    uint32_t adj_out[kBatchMax];  // sum_q ADJ[j][q]
    // (t,t) members (at most kTTMax per batch, in batch order): index and token of the first one (kNoTT: none) and
    // their number; their matches are every second token of a run of t, see tt_rename in kernels.hip
    uint32_t tt_index;
    uint32_t tt_token;
    uint32_t tt_n;
    // multiplier of the lookup-table hash for this batch: the selection tries several and keeps one under which no
    // bucket of the table has to hold a third key (kernels.hip: kHashMul, pair_hash)
    uint32_t hash_mul;
    // every member is a pair of raw bytes (ids below 256; a (t,t) member's second token is its stand-in): the stream
    // kernels then look pairs up in a direct table first byte x second byte instead of the hash table, which holds
    // any batch up to kBatchMax pairs (the hash table's buckets end batches near 1,400)
    uint32_t byte_lut;
    // candidates passed over because they depend on an earlier member of the batch (see k_sel_pick)
    uint32_t skip_n;
    uint32_t skip_key[kSkipMax];
    uint32_t skip_pos[kSkipMax];            // members accepted before it
    unsigned long long skip_packed[kSkipMax];
};

// exchange buffer (u32 words): [single-merge header: m, adj, RankEdge x n_ranks]
//   [batch header: m_j (kBatchMax), ADJ[i][j] (adj_pitch^2, row pitch DevCtl::adj_pitch)] [LR: rows L_0, R_0, L_1, R_1, ... of lr_pitch(ids) cells]
inline uint32_t batch_header_words(uint32_t adj_pitch) { return (uint32_t)kBatchMax + adj_pitch * adj_pitch; }
// row pitch of the LR block for a sequence that starts with `ids` token ids (256 + merges done): the ids rounded up
// to 64 cells, so that rows start on 256-byte lines.  A batch of n pairs touches the first 2 * n * pitch cells.
__host__ __device__ inline uint32_t lr_pitch(uint32_t ids) { return (ids + 63u) & ~63u; }
__host__ __device__ inline unsigned long long lr_words(uint32_t ids, uint32_t n_pairs) {
    return 2ull * (n_pairs ? n_pairs : 1u) * lr_pitch(ids);
}

constexpr uint32_t kErrTableFull   = 1u;
constexpr uint32_t kErrNegCount    = 2u;
constexpr uint32_t kErrMissingPair = 4u;
constexpr uint32_t kErrCountRange  = 8u;   // a pair count does not fit 31 bits (the table keeps a "present" flag in bit 31),
                                           //   or the byte-pair table does not add up to the pairs counted (k_pair_total)
constexpr uint32_t kErrHotSkipped  = 16u;  // a pass needed the frequent-pair instantiation of a stream kernel, which the host
                                           //   had ruled out and not launched (kernels.hip: hot_mismatch)
constexpr uint32_t kErrLog         = 32u;  // the delta log held more records of a bucket than its pairs' counts allow

// packed argmax word: (count << 32) | ~key  -- larger is better:
// count descending, then key ascending == (first, second) ascending,
// i.e. CompareLexicalOrder, PairCount.h:194-207.
__host__ __device__ inline unsigned long long pack_best(int32_t count, uint32_t key) {
    return ((unsigned long long)(uint32_t)count << 32) | (uint32_t)(~key);
}

// ---- kernel launchers (implemented in kernels.hip) ------------------------
// What every stream kernel needs is ONE StreamView, the buffers of a batch ONE BatchView (built in one place each:
// train.cpp, stream_view / batch_view); a launcher takes them plus only what is particular to that launch.
struct StreamView {
    hipStream_t stream;
    // seq == 0 (one merge per pass): the live buffer and the other one.  seq != 0 (inside a batch sequence): token
    // buffers 0 / 1, and ctl->cur picks the live one (a fused pass flips it without the host knowing)
    uint16_t *tok, *tok_other;
    TileSum *sums;           // live tile summaries
    TileSum *side;           // new summaries of the tiles a pass changed (launch_apply / launch_patch_sums fold them in)
    uint32_t n_tiles;
    uint32_t *chg;           // bitmap of those tiles
    uint32_t *tile_list;     // [n_tiles] scratch: the same as a dense list (launch_rewrite_marked)
    uint32_t *run_in;        // n_tiles entries: run of t before every tile, for (t,t) pairs
    unsigned long long *run_part;   // tile_scan_scratch(n_tiles) entries (the run kernels' chunk sums)
    DevCtl *ctl;
    const RankEdge *left_edge, *right_edge;   // composed neighbours of this rank's shard; NULL on one rank
    int rank, n_ranks;       // (n_ranks >= 1)
    uint32_t endbit;         // chunk-end convention: 0 (one chunk), kEndBit (flag in the slot) or kBarrier (barrier slots)
    int n_cus;
};

struct BatchView {
    BatchState *bs;
    uint32_t *hdr_m, *hdr_adj;   // batch header of the exchange buffer: m_j, ADJ[i][j]
    uint32_t *LR;                // count deltas: rows L_0, R_0, L_1, R_1, ... (one merge: L[x] = LR[2x], R[y] = LR[2y+1])
    // (optional) the delta log.  A match whose two neighbours are raw bytes and which no other match touches then costs
    // the scan / fused pass one 4-byte record in `dlog` instead of two atomics (L_j[x], R_j[y]); launch_log_consume, right
    // behind the pass, sorts the records by bucket into `part` and adds them to the LR rows: everything after it sees the
    // rows it always saw.  launch_log_plan, before the pass, lays out `part` and decides whether the pass logs.
    uint32_t *dlog, *part;
    LogState *ls;
};

// Which instantiations of a stream kernel a launch enqueues: they exist per (t,t) pair / member yes / no and per
// frequent pair (delta cache) yes / no, and each returns at once unless the pass is its case.  Not known: all of them, the
// frequent-pair ones only if `hot` (0: they cannot be needed).  Known (launch_seq_info told the host): exactly the one
// with this `tt` and `hot`.  `hot` is also what the kernels are told was launched (kErrHotSkipped: hot_mismatch).
struct Inst { bool known, tt, hot; };
inline Inst inst_any(bool hot_possible) { return Inst{false, false, hot_possible}; }
inline Inst inst_known(bool tt, bool hot) { return Inst{true, tt, hot}; }
// is the (tt, hot) instantiation among those `w` enqueues / any that handles a (t,t) pair?
inline bool inst_takes(const Inst &w, bool tt, bool hot) { return w.known ? w.tt == tt && w.hot == hot : !hot || w.hot; }
inline bool inst_may_tt(const Inst &w) { return !w.known || w.tt; }

void launch_fill_u32(hipStream_t s, uint32_t *p, uint64_t n, uint32_t v);
void launch_fill_u16(hipStream_t s, uint16_t *p, uint64_t n, uint16_t v);

// pair-count scan over the byte corpus. endmask: bit i set = byte i is the
// last byte of its chunk (NULL for a one-chunk corpus). bp[first<<8|second].
// scratch: pair_count_scratch_bytes(n_workgroups) of device memory (per-workgroup histogram snapshots)
size_t pair_count_scratch_bytes(int n_workgroups);
// start / stop (optional): HIP events recorded at the beginning and the end of the dispatch itself
void launch_pair_count_u8(hipStream_t s, const uint8_t *text, uint64_t n,
                          const uint8_t *endmask, uint32_t *bp, int n_workgroups, uint32_t *scratch,
                          hipEvent_t start = nullptr, hipEvent_t stop = nullptr);

// u8 corpus -> 16-bit slot stream (+END flags), padded to whole tiles with holes
void launch_widen(hipStream_t s, const uint8_t *text, uint64_t n, const uint8_t *endmask,
                  uint16_t *tok, uint64_t n_slots_padded);
// barrier layout: byte i -> slot 2i, slot 2i+1 = barrier or hole; n_slots = 2 * (n rounded up to 256)
void launch_widen_barrier(hipStream_t s, const uint8_t *text, uint64_t n, const uint8_t *endmask,
                          uint16_t *tok, uint64_t n_slots);

// recompute every tile summary from the slots of v.tok
void launch_summarize(const StreamView &v);

// dense byte-pair histogram -> pair table
void launch_table_init(hipStream_t s, const uint32_t *bp, PairTable t, DevCtl *ctl);
// rebuild the hash index from the entry arrays (after growing the table)
void launch_table_rehash(hipStream_t s, PairTable t, DevCtl *ctl);

// best[0] = max over entries of pack_best(count, key)   (best must be zeroed)
// hierarchical = one workgroup walking the block bounds (large tables); else a full scan
void launch_argmax(hipStream_t s, PairTable t, const DevCtl *ctl, unsigned long long *best, bool hierarchical);

// `first` tie-break (reference PairCountInsertOrder, PairCount.h:65-74, :101-181): after the argmax wrote
// best[0] = (max count, lexical winner), replace it by the pair of that count whose first occurrence in
// the stream comes first.  fs: first_state_bytes() of device memory, prepared once by launch_first_init.
size_t first_state_bytes();
void launch_first_init(hipStream_t s, void *fs);
// seq != 0: inside a batch sequence: best is the array, the merge index is ctl->k_done, and the kernels only work
// when the selection flagged a tie (ctl->first_tie).
// phase 0: one rank -- gather, position, pick.  Sharded stream: 1 = gather, position, publish this rank's earliest hit
// in its slot of xf (exchange_header_words(n_ranks) words); [sum xf over the ranks]; 2 = pick the hit of the lowest
// rank that has one.
void launch_first_tiebreak(const StreamView &v, PairTable t, unsigned long long *best, void *fs, uint32_t *xf, int seq,
                           int phase);

// one merge pass over the stream, in place; new summaries of changed tiles go to v.side, their bits are set in v.chg
// (launch_apply folds them into sums).  seq != 0: the kernel runs inside a batch sequence: it reads the merge index
// from ctl->k_done and returns at once unless the selected batch has one pair (which may be a (t,t) member of b.bs).
// m_adj: the [m, adj] accumulators.  w.tt: the pair is a (t,t) pair (run kernels).
void launch_merge(const StreamView &v, const BatchView &b, const unsigned long long *best, uint32_t new_id,
                  uint32_t *m_adj, int seq, const Inst &w);
// the run kernels launch_merge starts with, alone (a host that enqueues a batch's pass by itself: train.cpp, lockstep)
void launch_run_lengths(const StreamView &v, const BatchState *bs, const unsigned long long *best, int seq);

// fold the merge's count deltas (L, R, m, adj) into the pair table; gm_gadj: the [m, adj] summed over the ranks, or NULL;
// new_id: the id of the new token, or (seq != 0) an upper bound of it
void launch_apply(const StreamView &v, const BatchView &b, PairTable t, const unsigned long long *best, uint32_t new_id,
                  const uint32_t *gm_gadj, int seq);
// only the summary fold of launch_apply (multi-GPU: it must precede the rank edge)
void launch_patch_sums(const StreamView &v, const unsigned long long *best, int seq);

// ---- batched merges (see kernels.hip "batched merges") ----
// what a selection is asked for (train.cpp: select_args)
struct SelectArgs {
    SelList *sel;            // candidates of the threshold selection; NULL: the bound-walking kernel alone
    uint32_t n_target, max_batch, fused_min, sel_cap;
    bool byte_table;
};
// k_sel_scan + k_sel_pick (gather everything above a threshold, sort, take the independent
// prefix), then k_select_batch (walks the argmax bounds one pair at a time) if that could not be used
void launch_select_batch(const StreamView &v, const BatchView &b, PairTable t, unsigned long long *best,
                         const SelectArgs &a, int attempts = 3,
                         int first_attempt = 0 /* attempts first_attempt .. attempts - 1 */,
                         bool fallback = true /* the bound-walking kernel behind them */);
// (up to three gather + pick attempts are enqueued: when the first gather overflows its list -- many equal
//  counts -- the second lists the block bounds to find a threshold and the third gathers with it.  `attempts` 1: only
//  the first; the host enqueues the other two while selections have needed them lately)
// small batch: count the deltas and mark the tiles (the rewrite follows validation)
void launch_scan_batch(const StreamView &v, const BatchView &b, const Inst &w);
// large batch (ctl->fused): count the deltas and write the merged stream to the other buffer
void launch_fused_batch(const StreamView &v, const BatchView &b, const Inst &w);
// the delta log before / behind the pass (see BatchView; nothing to do without the log)
void launch_log_plan(const StreamView &v, const BatchView &b);
void launch_log_consume(const StreamView &v, const BatchView &b);
// k_delta_max + k_validate + k_apply_batch.  n_hint: the batch size the grids are sized for; id_upper: upper bound of
// the ids that exist
void launch_batch_tables(const StreamView &v, const BatchView &b, PairTable t, uint32_t id_upper, uint32_t n_hint);
// w: only whether the batch has a (t,t) member matters (v.run_in is used then, as for launch_merge)
void launch_rewrite_marked(const StreamView &v, const BatchView &b, const Inst &w);
// what the selection decided, for a host that enqueues only the kernels a sequence needs: out[0] merges done, [1] pairs
// in the batch, [2] fused pass, [3] a (t,t) pair among them, [4] frequent-pair instantiation, [5] merge limit,
// [6] the batch was chosen by a gather + pick attempt (0 after the first attempt alone: enqueue the others and the fallback)
void launch_seq_info(const StreamView &v, const BatchView &b, const unsigned long long *best, uint32_t *out);
// fused_flag (optional, 4 words): [0] = 1 when this sequence ran the fused pass, [1..2] = live tokens of the shard after
// the sequence, [3] = merges it committed
void launch_seq_finish(const StreamView &v, const BatchView &b, uint32_t *fused_flag);

// compaction: exclusive scan of n_live over tiles, then scatter.  `offsets` needs
// n_tiles + tile_scan_scratch(n_tiles) entries.
inline size_t tile_scan_scratch(uint32_t n_tiles) { return (size_t)n_tiles / 4096 + 2; }
void launch_tile_scan(const StreamView &v, unsigned long long *offsets);
// v.tok -> v.tok_other
void launch_compact_scatter(const StreamView &v, const unsigned long long *offsets);

// multi-GPU exchange header (u32 words): [0] m, [1] adj, [2 + 8r ..] RankEdge of rank r
inline uint32_t exchange_header_words(int n_ranks) { return (uint32_t)((2 + 8 * n_ranks + 3) / 4 * 4); }
// this rank's RankEdge from its tile summaries, into its place in the header (which also receives m, adj)
void launch_rank_edge(const StreamView &v, uint32_t *hdr);
// neighbours of this rank's shard from the gathered edges; clears the header
void launch_compose_edges(hipStream_t s, uint32_t *hdr, int rank, int n_ranks, RankEdge *left, RankEdge *right);
// the words that follow the header in the begin exchange: the number of pairs counted into the byte-pair table as four
// 16-bit limbs, one per u32 word, so that the u32 sum over the ranks cannot carry out of a limb
constexpr uint32_t kPairCountWords = 4;
// begin: pairs straddling rank boundaries -> byte-pair table, and their number added to pcount[0] (pcount != NULL)
void launch_boundary_pairs(hipStream_t s, uint32_t *bp, const uint32_t *hdr, int n_ranks, uint32_t endbit,
                           uint32_t *pcount);
// 64-bit sum of the byte-pair table against the number of pairs counted (expect + the limbs of pcount, when given):
// mismatch -> kErrCountRange in ctl->err (ctl != NULL); the sum -> *sum_out (sum_out != NULL)
void launch_pair_total(hipStream_t s, const uint32_t *bp, const uint32_t *pcount, unsigned long long expect,
                       unsigned long long *sum_out, DevCtl *ctl);

// ---- continuing from existing merges (mbpe_train_begin_from) ----
// `tok`: the n_tok 32-bit tokens the rank-ordered encoder leaves on the device, bit 31 = last token of its chunk.
// The pair counts are gathered in BINS first: the dense pair table's own cells (key == NULL), or -- hashed layout --
// an open-addressed table of the begin's own (mask + 1 slots, key filled with kEmptyKey, cnt with 0) that takes
// concurrent adds of a new pair, which the pair table's insert path does not.
struct PairBins { uint32_t *key, *cnt; uint32_t mask; };
// positions counted / sum and number of the bins / kErr* flags of the count kernel (zeroed by the host)
struct ResumeTally { unsigned long long positions, total; uint32_t distinct, err; };
// tokens -> 16-bit slots.  endbit 0 / kEndBit: slot i = token i, holes up to n_slots (a multiple of kTile).  kBarrier:
// sparse like launch_widen_barrier -- token i in slot 2i, its barrier or a hole behind it; n_slots = 2 * (n_tok rounded
// up to kTile / 2) -- for the compaction to squeeze
void launch_slots_from_tokens(hipStream_t s, const uint32_t *tok, uint64_t n_tok, uint32_t endbit, uint16_t *slots,
                              uint64_t n_slots);
// *n_ends += tokens that end a chunk
void launch_token_ends(hipStream_t s, const uint32_t *tok, uint64_t n_tok, unsigned long long *n_ends);
// every adjacent pair inside a chunk -> bins (LDS cache per workgroup, flushed once); ids: token ids that exist
void launch_pair_count_tokens(hipStream_t s, const uint32_t *tok, uint64_t n_tok, uint32_t ids, PairTable t, PairBins bins,
                              ResumeTally *tally, int n_cus);
// dense: raw counts in the cells -> present flags, ctl->n_entries, bmax / smax, tally->total / distinct
void launch_bins_seal_dense(hipStream_t s, PairTable t, uint32_t ids, DevCtl *ctl, ResumeTally *tally);
// hashed: tally->total / distinct of the bins; then every bin into the pair table (table_add, one thread per pair)
void launch_bins_tally(hipStream_t s, PairBins bins, ResumeTally *tally);
void launch_bins_insert(hipStream_t s, PairBins bins, PairTable t, DevCtl *ctl);
// total != positions -> kErrCountRange; the tally's flags -> ctl->err
void launch_resume_check(hipStream_t s, const ResumeTally *tally, DevCtl *ctl);

}  // namespace mbpe

#endif
