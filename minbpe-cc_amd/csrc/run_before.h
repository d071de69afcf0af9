// The run of equal raw tokens that ends just before a tile, from the tile summaries alone: what k_run_final
// (kernels.hip) stores in run_in[tile] for every tile of the stream, computed for ONE tile by walking the summaries
// back from it.  The split route of a fused pass asks for a fraction of a percent of the tiles, so it walks instead
// of scanning (kernels.hip: run_before_tile_wave is the same walk, 64 summaries per step).
//
// Usable on host and device, and free of HIP headers so that a host compiler can build it alone: the summary and
// edge types are template parameters (TileSum and RankEdge of mbpe_dev.h, or stand-ins of the same field names).
#ifndef MBPE_RUN_BEFORE_H
#define MBPE_RUN_BEFORE_H

#include <stdint.h>

#if defined(__HIPCC__)
#define MBPE_RB_HD __host__ __device__ inline
#else
#define MBPE_RB_HD inline
#endif

namespace mbpe {

constexpr uint32_t kRunNoToken = 0xFFFFu;        // (kHole: a rank edge without a token)

// The walk's state, going back from the tile: the run seen so far is `len` tokens equal (raw) to `token`;
// `open`: every non-empty tile seen was that run and nothing else, so the run may go on before it.
struct RunWalk {
    unsigned long long len;
    uint32_t token;
    bool started, open;
};
MBPE_RB_HD RunWalk run_walk_begin() { return RunWalk{0ull, 0u, false, false}; }

// One summary further back (tail0 raw, tail_run, n_live).  -> go on to the tile before it?
//   an empty tile is skipped; the nearest non-empty tile gives the token and its trailing run; a tile that is one
//   whole run (tail_run == n_live) continues into the tile before it only if that tile ends with the same raw token.
MBPE_RB_HD bool run_walk_take(RunWalk &w, uint32_t tail0, uint32_t tail_run, uint32_t n_live) {
    if (n_live == 0u) return true;
    if (w.started && tail0 != w.token) { w.open = false; return false; }
    w.started = true;
    w.token = tail0;
    w.len += tail_run;
    w.open = tail_run == n_live;
    return w.open;
}

// The walk is over (it stopped, or ran out of tiles): the left rank's trailing run is added while everything before
// the tile is that token (or nothing), as k_run_final's `reach`.  -> (run & 1) | (run >= 2 ? 2 : 0)
template <class Edge>
MBPE_RB_HD uint32_t run_walk_result(const RunWalk &w, const Edge *le) {
    unsigned long long rb = w.len;
    if (le && le->tail0 != kRunNoToken && (!w.started || (w.open && w.token == le->tail0)))
        rb += ((unsigned long long)le->tail_run_hi << 32) | le->tail_run_lo;
    return (uint32_t)(rb & 1ull) | (rb >= 2ull ? 2u : 0u);
}

// run_in[tile] of k_run_final, for one tile.  le: the left neighbour rank's edge, or null.
template <class Sum, class Edge>
MBPE_RB_HD uint32_t run_before_tile(const Sum *sums, uint32_t n_tiles, uint32_t tile, const Edge *le) {
    RunWalk w = run_walk_begin();
    if (tile > n_tiles) tile = n_tiles;
    while (tile > 0u) {
        const Sum &s = sums[--tile];
        if (!run_walk_take(w, s.tail0, s.tail_run, s.n_live)) break;
    }
    return run_walk_result(w, le);
}

}  // namespace mbpe

#endif
