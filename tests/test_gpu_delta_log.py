"""The delta log of the stream passes ("pair_cells" 1: forced on for every batch) against the oracle.

A match of a batch pair whose two neighbours are raw bytes, with both sides open and no other match touching it, is
written as one record (j << 16 | x << 8 | y) into a log; behind the pass the records are sorted into buckets of 64
pairs and counted in LDS.  Every case steps the training one sequence at a time and compares, after every sequence, the
merges, their counts and the whole pair table with an oracle state advanced by as many merges.  The cases aim at what
the log adds: several buckets and their edges, the chunk refill and the chunk tails, a log that is full, matches at
the edges of a tile, the matches that must stay out of the log, and batch sizes around a bucket boundary.

The frequent-pair instantiation of the stream kernels (a top pair that makes up 1 / 8192 of the stream or more) never
logs, so every corpus here keeps its pair counts below that: many distinct pairs, each of them rare."""
import numpy as np
import pytest

import mbpe
import oracle as O
from conftest import read_data

pytestmark = pytest.mark.gpu

OPTS = {"pair_cells": -1, "log_cap": 0, "log_chunk": 0, "fused_min": 24, "max_batch": 4096, "chunk_barrier": -1,
        "compact_den": 16, "lockstep": -1}


@pytest.fixture(scope="module")
def tr():
    t = mbpe.Trainer(0)
    yield t
    t.close()


def _keys(a, b):
    return (a.astype(np.uint64) << np.uint64(32)) | b.astype(np.uint64)


def _table(tr, ost, st, where):
    """The device's pair table as a set against the oracle's never-erased one (as test_gpu_stats compares it)."""
    a, b, c = tr.pairs()
    assert st["n_pairs"] == len(a), where
    oa, ob, oc = ost.table()
    order = np.argsort(_keys(oa, ob))
    ok, oa, ob, oc = _keys(oa, ob)[order], oa[order], ob[order], oc[order]
    order = np.argsort(_keys(a, b))
    dk, dc = _keys(a, b)[order], c[order]
    assert len(np.unique(dk)) == len(dk), "a pair is in the device table twice " + where
    pos = np.minimum(np.searchsorted(ok, dk), len(ok) - 1)
    extra = dk[ok[pos] != dk]
    assert len(extra) == 0, "device pairs the oracle never inserted %s: %s" % (
        where, [(int(k) >> 32, int(k) & 0xFFFFFFFF) for k in extra[:8]])
    differ = np.flatnonzero(dc != oc[pos])
    assert len(differ) == 0, "counts differ %s: %s" % (
        where, [(int(dk[i]) >> 32, int(dk[i]) & 0xFFFFFFFF, int(dc[i]), int(oc[pos[i]])) for i in differ[:8]])
    lacking = np.ones(len(ok), dtype=bool)
    lacking[pos] = False
    assert not np.any(oc[lacking]), "the device lacks pairs that occur " + where
    assert np.all((oa[lacking] >= 256) | (ob[lacking] >= 256)), "the device lacks a pair of raw bytes " + where


def _run(tr, data, off, vocab, **opts):
    """One training, a sequence at a time, against an oracle state; returns the merges of every sequence, the merge list
    and the final stats."""
    for k, v in dict(OPTS, pair_cells=1, **opts).items():
        tr.set_option(k, v)
    ost = O.State(data, off)
    try:
        tr.load_corpus(data, off)
        tr.train_begin(vocab)
        k, sizes = 0, []
        while True:
            d = tr.train_sequences(1)
            if d == 0:
                break
            tops = []
            for j in range(d):
                top = ost.top()
                assert top is not None
                tops.append(top)
                ost.merge(top[0], top[1], 256 + k + j)
            m, c = tr.train_result()
            where = "after merge %d (+%d)" % (k, d)
            assert len(m) == k + d, where
            assert [(int(m[k + j][0]), int(m[k + j][1]), int(c[k + j])) for j in range(d)] == tops, where
            st = tr.stats()
            assert st["n_live"] == len(ost.stream()[0]), where
            _table(tr, ost, st, where)
            k += d
            sizes.append(d)
        st = tr.stats()
        print("sequences", sizes[:12], "log_passes", st["log_passes"], "log_spilled", st["log_spilled"])
        assert k == vocab - 256
        return sizes, tr.train_result()[0], st
    finally:
        ost.close()
        for k, v in OPTS.items():
            tr.set_option(k, v)


# ---- several buckets, the chunk refill, the full log -----------------------------------------------------------------
def _units_corpus(n_bytes, seed=5):
    """Units `a b z`: a from 64 byte values, b from 64 others, z from the remaining 128.  Every one of the 4,096 pairs
    (a, b) occurs equally often -- about twice as often as any (b, z) or (z, a) at its luckiest -- and no two of them
    share a token on opposite sides: one batch can take them all, and nearly all their matches lie between raw bytes."""
    rng = np.random.default_rng(seed)
    A, B, Z = np.arange(32, 96), np.arange(96, 160), np.concatenate([np.arange(0, 32), np.arange(160, 256)])
    units = n_bytes // 3
    reps = units // 4096
    assert reps * 8192 < 3 * 4096 * reps          # (not the frequent-pair instantiation's)
    ab = np.repeat(np.arange(4096), reps)
    rng.shuffle(ab)
    out = np.empty((len(ab), 3), dtype=np.uint8)
    out[:, 0] = A[ab >> 6]
    out[:, 1] = B[ab & 63]
    out[:, 2] = Z[rng.integers(0, 128, size=len(ab))]
    return out.reshape(-1)


UNITS = _units_corpus(1 << 20)
UNITS_VOCAB = 256 + 4200


@pytest.mark.parametrize("case", ["buckets", "chunk_min", "log_full"])
def test_many_pairs(tr, case):
    """One chunk, thousands of pairs in a batch: the records of a pass spread over many buckets of 64 pairs.
    chunk_min: a wave reserves one tile's worth of records, the smallest chunk there is, and pads what its tile leaves
    of it (the 2,048 tiles of this corpus are one per wave: test_chunk_refill is where a wave comes back for more).
    log_full: the log holds 4,096 records, far less than one pass writes (4,096 pairs x 85 matches): most waves find
    it full and count with atomics instead -- the results are the same."""
    opts = {"buckets": {}, "chunk_min": {"log_chunk": 256}, "log_full": {"log_cap": 4096}}[case]
    sizes, m, st = _run(tr, UNITS, None, UNITS_VOCAB, **opts)
    assert max(sizes) >= 1024, sizes            # (else the corpus is wrong, not this line)
    assert st["log_passes"] > 0
    if case == "log_full":
        assert st["log_spilled"] > 0
    else:
        assert st["log_spilled"] == 0


# ---- a wave that fills its chunk and takes another -------------------------------------------------------------------
REFILL_UNITS = _units_corpus(3 * 4096 * 200, seed=7)


def test_chunk_refill(tr):
    """2.3 MiB, 4,800 tiles: more than a grid has waves (16 per compute unit and resident workgroup: 4,096 on 256
    compute units), so some 700 waves walk two tiles.  With chunks of 256 records and some 40 matches of the 1,024-pair
    batch in a tile, the second tile finds fewer than 256 records left: the wave pads the rest of its chunk and takes the
    next one, with its place in the log carried from tile to tile.  mbpe_stats.log_refills counts exactly those
    reservations.  The log is given room for a chunk per tile (4,800 x 256 records; the default for so short a stream
    is 2^20), so that no wave finds it full.  (1,024 pairs at a time and 1,100 merges keep the oracle's share of the
    test short.)"""
    sizes, m, st = _run(tr, REFILL_UNITS, None, 256 + 1100, log_chunk=256, log_cap=1 << 21, max_batch=1024)
    assert max(sizes) >= 1024, sizes
    assert st["log_passes"] > 0 and st["log_spilled"] == 0
    # (a device with 300 compute units or more -- 4,800 waves -- gives every tile a wave of its own: this line then
    #  fails, loudly, and the corpus has to grow with the grid)
    assert st["log_refills"] > 0


# ---- batch sizes around a bucket boundary ----------------------------------------------------------------------------
SMALL_UNITS = _units_corpus(3 * 4096 * 20)


@pytest.mark.parametrize("n_pairs", [2, 64, 65])
def test_batch_sizes(tr, n_pairs):
    """Batches of exactly 2, 64 and 65 pairs: one bucket that is nearly empty, one that is full, and pair 64 alone in a
    second one.  (The first batches end early at the few (z, a) pairs that chance made frequent; once the equal counts
    of the (a, b) pairs are reached a batch fills up to "max_batch".)"""
    sizes, m, st = _run(tr, SMALL_UNITS, None, 256 + 200, max_batch=n_pairs, fused_min=2)
    assert n_pairs in sizes and max(sizes) == n_pairs, sizes
    assert st["log_passes"] > 0 and st["log_spilled"] == 0


# ---- matches at the edges of a tile ----------------------------------------------------------------------------------
EDGE_SLOTS = (0, 510, 511)


def _edges_corpus():
    """64 KiB of 4-byte units `a b r r`: 2,304 pairs (a, b), seven units each, r a filler byte chosen in rotation so
    that no pair with a filler in it reaches seven.  Three sections, shifted by 0, 2 and 3 bytes: before the first
    merge a slot is a byte, so the units start at slots 0 / 2 / 3 (mod 4) of the 512-slot tiles.  The two pairs the
    first batch takes -- the smallest keys among the equal counts -- each have a unit at slot 0, at 510 and at 511:
    a match at 510 or 511 takes its right neighbour (at 511 its second token too) from the next tile, one at slot 0
    its left neighbour from the tile before."""
    rng = np.random.default_rng(11)
    A, B, R = np.arange(32, 80), np.arange(80, 128), np.arange(128, 256)
    ab = np.repeat(np.arange(48 * 48), 7)
    rng.shuffle(ab)
    units = len(ab)
    third = units // 3
    start = np.arange(units) * 4 + np.where(np.arange(units) >= third, 2, 0) + np.where(np.arange(units) >= 2 * third, 1, 0)
    taken = set()
    for pair in (0, 1):
        for slot in EDGE_SLOTS:
            u = next(int(i) for i in np.flatnonzero(start % 512 == slot) if int(i) not in taken and 0 < i < units - 1)
            v = next(int(i) for i in np.flatnonzero(ab == pair) if int(i) not in taken)
            ab[u], ab[v] = ab[v], ab[u]
            taken.add(u)
    u = np.empty((units, 4), dtype=np.uint8)
    u[:, 0] = A[ab // 48]
    u[:, 1] = B[ab % 48]
    # (the k-th unit with a given b is followed by filler k, the k-th unit before a given a preceded by filler k)
    nth_b, nth_a = np.zeros(48, dtype=np.int64), np.zeros(48, dtype=np.int64)
    for i in range(units):
        b, a_next = ab[i] % 48, ab[(i + 1) % units] // 48
        u[i, 2] = R[(nth_b[b] + 29 * b) % 128]
        u[i, 3] = R[(37 * nth_a[a_next] + 11 * a_next) % 128]
        nth_b[b] += 1
        nth_a[a_next] += 1
    flat = u.reshape(-1)
    fill = np.array([1, 2, 3], dtype=np.uint8)
    data = np.concatenate([flat[:third * 4], fill[:2], flat[third * 4:2 * third * 4], fill[2:], flat[2 * third * 4:]])
    assert 7 * 8192 < len(data)                   # (not the frequent-pair instantiation's)
    return data


@pytest.mark.parametrize("fused_min", [2, 1000])
def test_tile_edges(tr, fused_min):
    """fused_min 2: the fused pass; 1000: the counting pass of small batches, which shares the tile function."""
    data = _edges_corpus()
    for a, b in ((32, 80), (32, 81)):             # the first batch's pairs: where their matches start
        at = np.flatnonzero((data[:-1] == a) & (data[1:] == b))
        assert len(at) == 7 and set(EDGE_SLOTS) <= set(int(x) % 512 for x in at), (a, b, at % 512)
    sizes, m, st = _run(tr, data, None, 256 + 60, fused_min=fused_min, compact_den=0, max_batch=2)
    assert sizes[0] == 2, sizes
    assert [(int(a), int(b)) for a, b in m[:2]] == [(32, 80), (32, 81)]
    assert st["log_passes"] > 0 and st["log_spilled"] == 0
    assert (st["n_fused"] > 0) == (fused_min == 2)


# ---- what must stay out of the log -----------------------------------------------------------------------------------
def _excluded(case):
    rng = np.random.default_rng(23)
    if case == "touching":                  # a b a b between two fillers: the two matches of (a, b) touch
        ab = np.repeat(np.arange(4096), 5)
        rng.shuffle(ab)
        u = np.empty((len(ab), 6), dtype=np.uint8)
        u[:, 0] = u[:, 2] = 32 + (ab >> 6)
        u[:, 1] = u[:, 3] = 96 + (ab & 63)
        u[:, 4:] = rng.integers(160, 256, size=(len(ab), 2))
        return u.reshape(-1), None, 256 + 300, {}
    if case == "merged_neighbour":          # uniform bytes: after some hundred merges a neighbour is a merged token now and then
        return O.splitmix64_bytes(9, 1 << 18), None, 256 + 600, {}
    if case == "chunk_end":                 # the end flag in the slot (MODE 1): the token after a chunk's last one is no neighbour
        data = rng.integers(1, 256, size=1 << 18, dtype=np.uint8)
        cuts = np.cumsum(rng.integers(2, 10, size=len(data) // 2))
        off = np.concatenate([[0], cuts[cuts < len(data)], [len(data)]]).astype(np.uint64)
        return data, off, 256 + 300, {"chunk_barrier": 0}
    if case == "bytes_0_255":               # units a b z whose z -- x and y of the matches -- is 0 or 255 now and then
        data = _units_corpus(3 * 4096 * 10, seed=29)
        assert np.count_nonzero(data[2::3] == 0) > 100 and np.count_nonzero(data[2::3] == 255) > 100
        return data, None, 256 + 300, {}
    raise ValueError(case)


@pytest.mark.parametrize("case", ["touching", "merged_neighbour", "chunk_end", "bytes_0_255"])
def test_excluded_matches(tr, case):
    data, off, vocab, opts = _excluded(case)
    sizes, m, st = _run(tr, data, off, vocab, fused_min=2, **opts)
    assert any(d >= 2 for d in sizes), sizes
    assert st["log_passes"] > 0 and st["log_spilled"] == 0
