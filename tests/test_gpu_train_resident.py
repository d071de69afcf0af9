"""The training option "resident" (csrc/wide_resident.h: the 32-bit loop's merges in one workgroup) against the oracle
on the expanded corpus, and against the same training with the option off where it must fall back.  A case that
expects the kernel also asserts that its launches made every merge: a silent fallback fails."""
import os
import subprocess

import numpy as np
import pytest

import mbpe
import oracle as O
import dedup_cases as C
from conftest import GOLDEN, ROOT, read_data, read_golden
from test_gpu_train_weighted import MODES, _step_parity
from test_gpu_wide import _word_corpus

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "minbpe-cc_amd", "minbpe-cc")
MAX_TOKENS = 1 << 20          # "resident_max_tokens" of the cases that expect the kernel, whatever its default


@pytest.fixture
def tr():
    with mbpe.Trainer(0) as t:
        t.set_option("resident", 1)
        t.set_option("resident_max_tokens", MAX_TOKENS)
        yield t


def _cr(mode):
    return 1 if mode == O.LEXICAL else 0


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n_sym", [1, 2, 3, 4])
def test_parity_per_step(tr, n_sym, mode):
    # one letter: `a a a` runs of both parities; two: touching `abab`
    chunks = C.random_chunks(99 + n_sym, 3000, 12, n_sym)
    uniq, weights, _ = C.dedup(chunks)
    merges = _step_parity(tr, uniq, weights, chunks, 256 + 60, mode)
    assert tr.resident_stats()[0] == len(merges)
    # ... and the same merges when one launch makes all of them
    u_data, u_off = C.join(uniq)
    m, _, _ = tr.train(u_data, 256 + 60, u_off, conflict_resolution=_cr(mode), weights=weights)
    assert [tuple(x) for x in m.tolist()][:len(merges)] == merges
    assert tr.resident_stats()[0] == len(m) and tr.decode_stream() == u_data.tobytes()


def _short_chunks():
    # 72 distinct chunks of one and two bytes: 136 tokens, regions of 9 whose boundaries fall on both kinds
    rng = np.random.default_rng(3)
    letters = [bytes([c]) for c in b"abcdefgh"]
    uniq = letters + [x + y for x in letters for y in letters]
    uniq = [uniq[i] for i in rng.permutation(len(uniq))]
    return uniq, rng.integers(1, 6, size=len(uniq)).astype(np.uint32)


def _collapsing_chunks():
    # fewer chunks than waves, and chunks that end as one token: regions empty from the start, regions left without a pair
    uniq = [b"ab" * k for k in (1, 2, 4, 8)] + [b"cd" * k for k in (1, 2, 4)] + [b"abcd", b"e"]
    return uniq, np.arange(1, len(uniq) + 1).astype(np.uint32)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("corpus", [_short_chunks, _collapsing_chunks])
def test_region_edges(tr, corpus, mode):
    uniq, weights = corpus()
    full = [uniq[i] for i in np.repeat(np.arange(len(uniq)), weights)]
    merges = _step_parity(tr, uniq, weights, full, 256 + 12, mode)
    assert tr.resident_stats()[0] == len(merges)


@pytest.mark.parametrize("cr", [1, 0], ids=["lexical", "first"])
def test_fewer_chunks_than_waves_at_the_count_limit(tr, cr):
    data = np.frombuffer(b"abab?", dtype=np.uint8)
    off = np.array([0, 2, 5], dtype=np.uint64)
    m, c, _ = tr.train(data, 256 + 2, off, conflict_resolution=cr, weights=[1 << 30, (1 << 30) - 1])
    assert m.tolist() == [[97, 98], [256, 63]] and c.tolist() == [(1 << 31) - 1, (1 << 30) - 1]
    assert tr.resident_stats()[0] == 2


@pytest.mark.parametrize("mode", MODES)
def test_unweighted(tr, mode):
    # load_corpus with offsets, no weights, handed over from the slot stream before its first merge
    data, off = C.join(C.random_chunks(7, 2000, 12, 3))
    want_m, want_c = O.train(data, 256 + 60, off, mode)
    tr.set_option("wide_from", 0)
    tr.set_option("first_wide", 1)
    m, c, _ = tr.train(data, 256 + 60, off, conflict_resolution=_cr(mode))
    assert m.tolist() == want_m.tolist() and c.tolist() == want_c.tolist()
    assert tr.resident_stats()[0] == len(m) and tr.decode_stream() == data.tobytes()


@pytest.mark.parametrize("mode", MODES)
def test_zero_count_tail(tr, mode):
    data = read_data("small.txt")
    chunks = C.chunks_of(data, mbpe.presplit(O.GPT4_SPLIT_PATTERN, data))
    uniq, weights, _ = C.dedup(chunks)
    vocab = 256 + len(data)
    f_data, f_off = C.join(chunks)
    want_m, want_c = O.train(f_data, vocab, f_off, mode)
    u_data, u_off = C.join(uniq)
    m, c, _ = tr.train(u_data, vocab, u_off, conflict_resolution=_cr(mode), weights=weights)
    assert m.tolist() == want_m.tolist() and c.tolist() == want_c.tolist()
    assert tr.resident_stats()[0] == len(m)
    if mode == O.LEXICAL:
        assert len(m) == vocab - 256 and int(c[-1]) == 0
    else:
        assert 0 < len(m) < vocab - 256 and int(c[-1]) > 0


def _both(tr, run):
    """run() with the option off, then on -> (results off, results on)"""
    tr.set_option("resident", 0)
    off = run()
    tr.set_option("resident", 1)
    return off, run()


@pytest.mark.parametrize("mode", MODES)
def test_table_growth_over_several_launches(tr, mode):
    data, off = _word_corpus(78, 1500, 16, (2, 5))
    uniq, weights, _ = C.dedup(C.chunks_of(data, off))
    u_data, u_off = C.join(uniq)

    def run():
        m, c, st = tr.train(u_data, 256 + 12000, u_off, conflict_resolution=_cr(mode), weights=weights)
        return m.tolist(), c.tolist(), tr.stream()[0].tolist(), st["n_table_grows"]

    want, got = _both(tr, run)
    assert got[:3] == want[:3]
    n_res, n_launches, _ = tr.resident_stats()
    assert n_res == len(got[0]) and n_launches > 1 and got[3] > 0


@pytest.mark.parametrize("why", ["max_tokens", "long_chunk", "min_frequency"])
def test_fallbacks_give_the_same_merges(tr, why):
    uniq = [b"ab" * 35000, b"abc"] if why == "long_chunk" else C.dedup(C.random_chunks(11, 500, 10, 3))[0]
    weights = np.arange(1, len(uniq) + 1).astype(np.uint32)
    u_data, u_off = C.join(uniq)
    if why == "max_tokens":
        tr.set_option("resident_max_tokens", len(uniq) - 1)      # (below any length the stream can shrink to)
    if why == "min_frequency":
        tr.set_option("min_frequency", 2)

    def run():
        m, c, _ = tr.train(u_data, 256 + 20, u_off, conflict_resolution=0, weights=weights)
        return m.tolist(), c.tolist(), tr.stream()[0].tolist()

    want, got = _both(tr, run)
    assert got == want and len(got[0]) > 10
    assert tr.resident_stats()[0] == 0


@pytest.mark.parametrize("mode", MODES)
def test_continuation_from_prior_merges(tr, mode):
    chunks = C.random_chunks(21, 3000, 10, 4)
    uniq, weights, _ = C.dedup(chunks)
    u_data, u_off = C.join(uniq)
    part_m, _, _ = tr.train(u_data, 256 + 20, u_off, conflict_resolution=_cr(mode), weights=weights)
    merges = _step_parity(tr, uniq, weights, chunks, 256 + 30, mode, prior=part_m)
    assert tr.resident_stats()[0] == len(merges) - 20 == 10


@pytest.mark.parametrize("cr", [1, 0], ids=["lexical", "first"])
def test_tokenizer_and_cli(tmp_path, cr):
    name = "lexical" if cr else "first"
    tok = mbpe.Tokenizer(O.GPT4_SPLIT_PATTERN)
    tok.train(read_data("taylorswift.txt"), 512, conflict_resolution=cr, dedup=True, resident=True)
    tok.save(str(tmp_path / "tok.model"))
    assert (tmp_path / "tok.model").read_bytes() == read_golden("taylorswift_gpt4_%s_512.model" % name)
    sample = os.path.join(GOLDEN, "data", "sample.txt")
    for out, flags in (("plain.model", []), ("resident.model", ["--dedup", "--resident"])):
        r = subprocess.run([CLI, "--train"] + flags + ["-i", sample, "-m", str(tmp_path / out), "-c", name,
                                                        "--vocab-size", "400"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
    assert (tmp_path / "resident.model").read_bytes() == (tmp_path / "plain.model").read_bytes()
