"""mbpe_stats against what the oracle knows after k merges: the stream length and the pair table.

The device is asked one batch sequence at a time (mbpe_train_sequences(1)) how many merges it committed; an oracle state
of the same corpus is advanced by as many, and every counter of mbpe_stats must then be what that sequence accounts for:
one pass, one size_hist bucket, the live tokens the oracle has, and -- with the option "time_kernels" -- the launch, slot
and live-token sums bench.py --full builds its roofline from.  The pair table is compared as a set: its members, their
counts (zeros included) and its lexicographic minimum, which the zero-count tail of a training depends on."""
import numpy as np
import pytest

import mbpe
import oracle as O
from conftest import read_data

pytestmark = pytest.mark.gpu

TILE = 512          # slots per tile: a compacted stream is padded to whole tiles

DEFAULTS = {"compact_den": 16, "batch": 16, "multi_merge": 1, "max_batch": 4096, "fused_min": 24, "hier_argmax": -1,
            "dense_table": -1, "threshold_select": 1, "sel_cap": 8192, "chunk_barrier": -1, "first_batches": 0, "byte_table": 1,
            "wide_from": -1, "lockstep": -1, "pair_cells": -1, "time_kernels": 0}

CUTS = ("cut_conflict", "cut_bucket", "cut_single", "cut_full", "n_validation_drops")
# what a training accounts for on the device, whichever way the host groups its sequences
DEVICE_COUNTERS = ("n_batches", "n_fused", "n_fused_dropped", "size_hist", "cut_conflict", "cut_bucket", "cut_single",
                   "cut_full")
# every field that only a training sets (n_bytes and n_chunks belong to the loaded corpus)
TRAINING_FIELDS = [name for name, _ in mbpe.Stats._fields_ if name not in ("n_bytes", "n_chunks")]


@pytest.fixture(scope="module")
def tr():
    t = mbpe.Trainer(0)
    yield t
    t.close()


def _defaults(tr):
    for k, v in DEFAULTS.items():
        tr.set_option(k, v)


def _keys(a, b):
    return (a.astype(np.uint64) << np.uint64(32)) | b.astype(np.uint64)


def _membership(tr, ost, st, where):
    """The device's pair table as a set against the oracle's never-erased one."""
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
    # (the transient (X,a) between two touching matches: count 0 again when the merge is over, X a merged token)
    assert not np.any(oc[lacking]), "the device lacks pairs that occur " + where
    assert np.all((oa[lacking] >= 256) | (ob[lacking] >= 256)), "the device lacks a pair of raw bytes " + where
    assert len(dk) and dk[0] == ok[0], "the tables' lexicographic minima differ " + where


def _bucket(d):
    return min(7, int(d).bit_length() - 1)


def _trace(tr, data, off, vocab, membership=True, wide_from=None, **opts):
    """Steps a training one sequence at a time; asserts every counter after every call; returns the per-call records
    (merges committed, stats after the call, whether the call ran on the slot stream) and the final stats."""
    for k, v in opts.items():
        tr.set_option(k, v)
    if wide_from is not None:
        tr.set_option("wide_from", wide_from)
    tr.set_option("time_kernels", 1)
    ost = O.State(data, off)
    try:
        tr.load_corpus(data, off)
        tr.train_begin(vocab)
        s = tr.stats()
        for name in ("n_merges", "n_batches", "n_fused", "merge_launches", "fused_launches"):
            assert s[name] == 0, name
        assert s["size_hist"] == [0] * 8
        n_chunks = 1 if off is None else len(off) - 1
        assert s["n_chunks"] == n_chunks and s["n_bytes"] == len(data)
        barrier = tr.stream_device()[4] is not None
        bar = n_chunks if barrier else 0            # barrier slots: in the stream, no tokens
        live = len(ost.stream()[0])
        assert s["n_live"] == live == len(data) and s["n_slots"] >= live + bar
        den = opts.get("compact_den", DEFAULTS["compact_den"])
        live_at_compaction = live
        k, calls, slot_batches = 0, [], 0
        while True:
            p = s
            d = tr.train_sequences(1)
            s = tr.stats()
            where = "after merge %d (+%d)" % (k, d)
            if d == 0:
                # nothing ran: a finished training accounts for nothing more
                for name in TRAINING_FIELDS:
                    if not name.startswith("ms_"):
                        assert s[name] == p[name], (name, where)
                break
            tops = []
            for j in range(d):
                top = ost.top()
                assert top is not None, where
                tops.append(top)
                ost.merge(top[0], top[1], 256 + k + j)
            m, c = tr.train_result()
            assert len(m) == k + d, where
            assert [(int(m[k + j][0]), int(m[k + j][1]), int(c[k + j])) for j in range(d)] == tops, where
            live_before, live = live, len(ost.stream()[0])
            on_slots = wide_from is None or k < wide_from
            k += d
            calls.append((d, s, on_slots))
            print(where, {n: s[n] for n in ("n_batches", "n_fused", "n_fused_dropped", "n_live", "n_slots", "n_pairs",
                                            "n_compactions", "merge_launches", "fused_launches", "fused_slots",
                                            "fused_live_tokens")})
            assert s["n_merges"] == k, where
            assert s["n_batches"] == p["n_batches"] + 1, where
            assert s["n_live"] == live, where
            if membership:
                _membership(tr, ost, s, where)
            if not on_slots:
                # the 32-bit continuation: one merge per pass on a stream without holes
                assert d == 1 and s["n_slots"] == live, where
                assert s["n_batches"] == slot_batches + (k - wide_from), where
                continue
            slot_batches = s["n_batches"]
            # ---- merge counters
            grown = [x - y for x, y in zip(s["size_hist"], p["size_hist"])]
            want = [0] * 8
            want[_bucket(d)] = 1
            assert grown == want, (d, grown, where)
            assert sum(s["size_hist"]) == s["n_batches"], where
            fused = s["n_fused"] - p["n_fused"]
            assert fused in (0, 1), where
            assert 0 <= s["n_fused_dropped"] - p["n_fused_dropped"] <= fused, where
            for name in CUTS:
                assert s[name] >= p[name], (name, where)
            if d >= 2 and opts.get("fused_min") == 2:
                assert fused == 1, where
            if opts.get("fused_min", 0) >= 1000:
                assert s["n_fused"] == 0, where
            # ---- the stream: "compact_den" compacts when holes * den >= slots, to whole tiles
            assert s["n_slots"] >= live + bar, where
            holes = live_at_compaction - live
            compacted = den > 0 and holes > 0 and holes * den >= p["n_slots"]
            assert s["n_compactions"] - p["n_compactions"] == int(compacted), (holes, p["n_slots"], where)
            if compacted:
                assert s["n_slots"] == max(-(-(live + bar) // TILE) * TILE, TILE), where
                live_at_compaction = live
            else:
                assert s["n_slots"] == p["n_slots"], where
            # ---- launch accounting (before the housekeeping that may compact)
            assert s["merge_launches"] - p["merge_launches"] == 1, where
            assert s["fused_launches"] - p["fused_launches"] == fused, where
            assert s["fused_slots"] - p["fused_slots"] == fused * p["n_slots"], where
            assert s["fused_live_tokens"] - p["fused_live_tokens"] == fused * (live_before + live + 2 * bar), where
            # ---- timers
            if not fused:
                assert s["ms_fused_kernel"] == p["ms_fused_kernel"], where
            assert s["ms_merge_kernel"] >= s["ms_fused_kernel"], where
        return calls, s
    finally:
        ost.close()
        _defaults(tr)


RANDOM_BYTES = O.splitmix64_bytes(3, 1 << 18)
RANDOM_VOCAB = 256 + 400


# fused_min 2: every multi-pair batch takes the fused pass; 1000: none does.  dense_table: one cell per possible pair /
# the hashed table.  compact_den 3 cannot trigger here -- 400 merges remove some 4,300 of the 262,144 tokens, a third
# of the slots would have to be holes -- so the trace asserts that it does not; 100 compacts near merge 240.
@pytest.mark.parametrize("den", [0, 3, 100])
@pytest.mark.parametrize("dense", [0, 1])
@pytest.mark.parametrize("fused_min", [2, 1000])
def test_trace_random_bytes(tr, fused_min, dense, den):
    calls, st = _trace(tr, RANDOM_BYTES, None, RANDOM_VOCAB, fused_min=fused_min, dense_table=dense, compact_den=den)
    assert st["n_merges"] == RANDOM_VOCAB - 256
    assert any(d >= 2 for d, _, _ in calls)                 # batches were formed
    assert (st["n_fused"] > 0) == (fused_min == 2)
    if den == 100:
        assert st["n_compactions"] >= 1
    if den == 3:
        assert st["n_compactions"] == 0


def _small_alphabet():
    return np.random.default_rng(17).integers(97, 100, size=6000, dtype=np.uint8)


# three symbols: (t,t) pairs, touching matches and their transient pairs, and a stream that loses two thirds of its
# tokens: with compact_den 3 it is compacted more than once.  threshold_select 0: the bound-walking selection, which
# merges every (t,t) pair alone (cut_single); 1, the default, gives such a pair a stand-in id and keeps it in the batch
@pytest.mark.parametrize("den,threshold_select", [(3, 0), (0, 0), (3, 1)])
def test_trace_small_alphabet(tr, den, threshold_select):
    data = _small_alphabet()
    calls, st = _trace(tr, data, None, 256 + 40, compact_den=den, fused_min=2, threshold_select=threshold_select)
    assert st["n_merges"] == 40
    m = tr.train_result()[0]
    assert any(int(a) == int(b) for a, b in m)              # (t,t) pairs were merged
    if threshold_select == 0:
        assert st["cut_single"] > 0
    assert (st["n_compactions"] >= 1) == (den == 3)


# chunk_barrier 0: a slot bit marks the last token of a chunk; 1: a barrier slot follows every chunk.  n_live counts
# tokens either way; fused_live_tokens counts what the pass reads and writes, barrier slots included (_trace)
@pytest.mark.parametrize("barrier", [0, 1])
def test_trace_chunked_text(tr, barrier):
    data = read_data("taylorswift.txt")[:60000]
    off = mbpe.presplit(O.GPT4_SPLIT_PATTERN, data)
    calls, st = _trace(tr, data, off, 256 + 150, fused_min=2, chunk_barrier=barrier)
    assert st["n_merges"] == 150 and st["n_chunks"] == len(off) - 1
    assert st["n_fused"] > 0 and st["fused_live_tokens"] > 0


def test_trace_abandoned_fused_pass(tr):
    """A run of 64 tiles of one byte before a text: the text's batches are cut by validation, and a fused pass whose
    batch was cut is abandoned (the kept prefix is applied to the current buffer).  Such a sequence still ran the pass:
    it counts in n_fused and fused_launches, and its live tokens after are the oracle's after the committed prefix."""
    text = read_data("shakespeare.txt")[3000:27000]
    data = np.frombuffer(b"a" * (512 * 64) + text, dtype=np.uint8)
    calls, st = _trace(tr, data, None, 256 + 400, compact_den=0, fused_min=2, lockstep=0)
    assert st["n_merges"] == 400
    assert st["n_fused_dropped"] > 0
    assert st["fused_launches"] == st["n_fused"] > st["n_fused_dropped"]


def test_trace_wide_continuation(tr):
    """The hand-over to 32-bit tokens after 30 merges ("wide_from"): from there on one merge per pass on a compacted
    stream; n_merges and n_batches go on counting across the hand-over."""
    calls, st = _trace(tr, _small_alphabet(), None, 256 + 40, wide_from=30, compact_den=0, fused_min=2)
    assert st["n_merges"] == 40
    assert [d for d, _, on_slots in calls if not on_slots] == [1] * 10
    assert sum(d for d, _, on_slots in calls if on_slots) == 30
    assert st["n_live"] == st["n_slots"]


def test_zero_count_tail_takes_no_passes(tr):
    """Pairs run out long before the vocabulary is full: PairCountLexicalOrder never erases, so the reference goes on
    choosing the smallest zero-count pair.  The device commits it once and fills in the rest without a pass each."""
    data = np.frombuffer(b"abcabdabcabd" * 40 + b"xyz", dtype=np.uint8)
    vocab = 256 + 3000
    want_m, want_c = O.train(data, vocab)
    real = int(np.count_nonzero(want_c))
    assert 0 < real < 40 and not np.any(want_c[real:])
    tr.set_option("time_kernels", 1)
    try:
        tr.load_corpus(data)
        tr.train_begin(vocab)
        k, s, zero_seen = 0, tr.stats(), False
        while True:
            p = s
            d = tr.train_sequences(1)
            s = tr.stats()
            print(k, d, s["n_batches"], s["merge_launches"], s["fused_launches"])
            if zero_seen:           # the chosen count has been 0: no pass, no launch any more
                for name in ("n_batches", "merge_launches", "fused_launches"):
                    assert s[name] == p[name], (name, k)
            if d == 0:
                break
            k += d
            assert s["n_merges"] == k
            zero_seen = k > real
        m, c = tr.train_result()
    finally:
        _defaults(tr)
    assert k == vocab - 256 == s["n_merges"]
    assert m.tolist() == want_m.tolist() and c.tolist() == want_c.tolist()
    # a pass commits at least one merge: the real merges, and the one pass that committed the first zero-count pair
    assert s["n_batches"] <= real + 1
    assert s["merge_launches"] == s["n_batches"] and s["fused_launches"] == s["n_fused"]


# ---- a whole training in one call ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stepped(tr):
    """The stepped trace of the random-bytes corpus with the options of the whole-training cases."""
    calls, st = _trace(tr, RANDOM_BYTES, None, RANDOM_VOCAB, membership=False, fused_min=2, compact_den=0)
    return st


@pytest.mark.parametrize("lockstep", [1, 0])
@pytest.mark.parametrize("batch", [2, 3, 5, 16])
def test_whole_training_accounts_like_the_stepped_trace(tr, stepped, batch, lockstep):
    """mbpe_train_begin + mbpe_train_steps(all) twice on one context, as bench.py does; the second training's share of
    the accumulated launch counters against the device's own counters of that training.  With "lockstep" 1 the host
    meets a sequence with nothing left to merge whenever the last group is not full: no k_seq_finish runs for it, and
    its timing record once was whatever an earlier sequence -- of the first training, in a reused buffer -- had left
    there: a phantom fused pass."""
    for k, v in {"fused_min": 2, "compact_den": 0, "batch": batch, "lockstep": lockstep, "time_kernels": 1}.items():
        tr.set_option(k, v)
    try:
        tr.load_corpus(RANDOM_BYTES)
        for _ in range(2):
            tr.train_begin(RANDOM_VOCAB)
            s0 = tr.stats()
            assert tr.train_steps(RANDOM_VOCAB - 256) == RANDOM_VOCAB - 256
            s1 = tr.stats()
    finally:
        _defaults(tr)
    print(batch, lockstep, {n: (s0[n], s1[n]) for n in ("fused_launches", "merge_launches", "fused_slots",
                                                        "fused_live_tokens", "n_fused", "n_batches")})
    assert s0["n_batches"] == 0 and s0["fused_launches"] == stepped["n_fused"]      # (the first training's are kept)
    assert s1["n_compactions"] == 0
    assert s1["fused_launches"] - s0["fused_launches"] == s1["n_fused"]
    assert s1["merge_launches"] - s0["merge_launches"] == s1["n_batches"]
    assert sum(s1["size_hist"]) == s1["n_batches"]
    assert s1["fused_slots"] - s0["fused_slots"] == s1["n_fused"] * s1["n_slots"]
    assert s1["fused_live_tokens"] - s0["fused_live_tokens"] == stepped["fused_live_tokens"]
    assert s1["ms_merge_kernel"] >= s1["ms_fused_kernel"] >= s0["ms_fused_kernel"]
    # batches are chosen on the device: how the host groups the sequences does not show
    for name in DEVICE_COUNTERS:
        assert s1[name] == stepped[name], name
    assert s1["n_live"] == stepped["n_live"] and s1["n_pairs"] == stepped["n_pairs"]


# ---- before mbpe_train_begin ------------------------------------------------------------------------------------
def test_stats_after_load_corpus_alone(tr):
    data = b"hello world\x00123abc"
    off = np.array([0, 5, 11, 15, 18], dtype=np.uint64)        # "\x00123": one token in the reference, no pair ever
    tr.set_option("time_kernels", 1)
    try:
        tr.train_lexical(RANDOM_BYTES[:4096], 256 + 20)            # (something to forget)
        tr.load_corpus(data, off)
        s = tr.stats()
        assert s["n_bytes"] == len(data) and s["n_chunks"] == 3
        for name in TRAINING_FIELDS:
            assert s[name] == ([0] * 8 if name == "size_hist" else 0), name
        tr.load_corpus(data)
        s = tr.stats()
        assert s["n_bytes"] == len(data) and s["n_chunks"] == 1
        for name in TRAINING_FIELDS:
            assert s[name] == ([0] * 8 if name == "size_hist" else 0), name
    finally:
        _defaults(tr)
