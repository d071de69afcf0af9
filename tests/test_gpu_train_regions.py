"""The training option "regions" (csrc/wide_regions.h: the 32-bit loop's merges on wave-owned regions, two launches per
merge) against the oracle on the expanded corpus, and against the same training with the option off where it must fall
back.  Regions of 64 tokens, so that a few thousand tokens make many of them.  A case that expects the route also
asserts that its groups made every merge: a silent fallback fails."""
import os
import subprocess

import numpy as np
import pytest

import mbpe
import oracle as O
import dedup_cases as C
from conftest import GOLDEN, ROOT, read_data, read_golden
from test_gpu_train_resident import _collapsing_chunks, _short_chunks
from test_gpu_train_weighted import MODES, _step_parity
from test_gpu_wide import _word_corpus

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "minbpe-cc_amd", "minbpe-cc")


@pytest.fixture
def tr():
    with mbpe.Trainer(0) as t:
        t.set_option("regions", 1)
        t.set_option("region_tokens", 64)
        yield t


def _cr(mode):
    return 1 if mode == O.LEXICAL else 0


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n_sym", [1, 2, 3, 4])
def test_parity_per_step(tr, n_sym, mode):
    # one letter: `a a a` runs of both parities; two: touching `abab`; candidates at both ends of many regions.
    # Every step is a group of one: cut, merge, close
    chunks = C.random_chunks(99 + n_sym, 3000, 12, n_sym)
    uniq, weights, _ = C.dedup(chunks)
    merges = _step_parity(tr, uniq, weights, chunks, 256 + 60, mode)
    assert tr.regions_stats()[0] == len(merges)
    # ... and the same merges when many of them rewrite the regions in place before one close
    u_data, u_off = C.join(uniq)
    m, _, _ = tr.train(u_data, 256 + 60, u_off, conflict_resolution=_cr(mode), weights=weights)
    assert [tuple(x) for x in m.tolist()][:len(merges)] == merges
    assert tr.regions_stats()[0] == len(m) and tr.decode_stream() == u_data.tobytes()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("corpus", [_short_chunks, _collapsing_chunks])
def test_region_edges(tr, corpus, mode):
    uniq, weights = corpus()
    full = [uniq[i] for i in np.repeat(np.arange(len(uniq)), weights)]
    merges = _step_parity(tr, uniq, weights, full, 256 + 12, mode)
    assert tr.regions_stats()[0] == len(merges)


@pytest.mark.parametrize("mode", MODES)
def test_unweighted(tr, mode):
    # load_corpus with offsets, no weights, handed over from the slot stream before its first merge
    data, off = C.join(C.random_chunks(7, 2000, 12, 3))
    want_m, want_c = O.train(data, 256 + 60, off, mode)
    tr.set_option("wide_from", 0)
    tr.set_option("first_wide", 1)
    m, c, _ = tr.train(data, 256 + 60, off, conflict_resolution=_cr(mode))
    assert m.tolist() == want_m.tolist() and c.tolist() == want_c.tolist()
    assert tr.regions_stats()[0] == len(m) and tr.decode_stream() == data.tobytes()


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
    assert tr.regions_stats()[0] == len(m)
    if mode == O.LEXICAL:
        assert len(m) == vocab - 256 and int(c[-1]) == 0
    else:
        assert 0 < len(m) < vocab - 256 and int(c[-1]) > 0


def _both(tr, run):
    """run() with the option off, then on -> (results off, results on)"""
    tr.set_option("regions", 0)
    off = run()
    tr.set_option("regions", 1)
    return off, run()


@pytest.mark.parametrize("mode", MODES)
def test_table_growth_over_several_groups(tr, mode):
    data, off = _word_corpus(78, 1500, 16, (2, 5))
    uniq, weights, _ = C.dedup(C.chunks_of(data, off))
    u_data, u_off = C.join(uniq)

    def run():
        m, c, st = tr.train(u_data, 256 + 12000, u_off, conflict_resolution=_cr(mode), weights=weights)
        return m.tolist(), c.tolist(), tr.stream()[0].tolist(), st["n_table_grows"]

    want, got = _both(tr, run)
    assert got[:3] == want[:3]
    n_reg, n_groups, _ = tr.regions_stats()
    assert n_reg == len(got[0]) and n_groups > 1 and got[3] > 0


@pytest.mark.parametrize("why", ["long_chunk", "min_frequency"])
def test_fallbacks_give_the_same_merges(tr, why):
    uniq = [b"ab" * 35000, b"abc"] if why == "long_chunk" else C.dedup(C.random_chunks(11, 500, 10, 3))[0]
    weights = np.arange(1, len(uniq) + 1).astype(np.uint32)
    u_data, u_off = C.join(uniq)
    if why == "min_frequency":
        tr.set_option("min_frequency", 2)

    def run():
        m, c, _ = tr.train(u_data, 256 + 20, u_off, conflict_resolution=0, weights=weights)
        return m.tolist(), c.tolist(), tr.stream()[0].tolist()

    want, got = _both(tr, run)
    assert got == want and len(got[0]) > 10
    assert tr.regions_stats()[0] == 0


@pytest.mark.parametrize("mode", MODES)
def test_hand_over_to_resident(tr, mode):
    # both options on: regions while the stream is longer than "resident_max_tokens", the one workgroup from there on
    uniq, weights, _ = C.dedup(C.random_chunks(21, 3000, 10, 4))
    u_data, u_off = C.join(uniq)

    def run():
        m, c, _ = tr.train(u_data, 256 + 200, u_off, conflict_resolution=_cr(mode), weights=weights)
        return m.tolist(), c.tolist(), tr.stream()[0].tolist()

    tr.set_option("regions", 0)
    want = run()
    first_len, last_len = len(u_data), len(want[2])
    assert last_len + 1 < first_len
    tr.set_option("regions", 1)
    tr.set_option("resident", 1)
    tr.set_option("resident_max_tokens", (first_len + last_len) // 2)
    assert run() == want
    n_reg, n_res = tr.regions_stats()[0], tr.resident_stats()[0]
    assert n_reg > 0 and n_res > 0 and n_reg + n_res == len(want[0])


@pytest.mark.parametrize("mode", MODES)
def test_continuation_from_prior_merges(tr, mode):
    chunks = C.random_chunks(21, 3000, 10, 4)
    uniq, weights, _ = C.dedup(chunks)
    u_data, u_off = C.join(uniq)
    part_m, _, _ = tr.train(u_data, 256 + 20, u_off, conflict_resolution=_cr(mode), weights=weights)
    merges = _step_parity(tr, uniq, weights, chunks, 256 + 30, mode, prior=part_m)
    assert tr.regions_stats()[0] == len(merges) - 20 == 10


@pytest.mark.parametrize("cr", [1, 0], ids=["lexical", "first"])
def test_tokenizer_and_cli(tmp_path, cr):
    name = "lexical" if cr else "first"
    tok = mbpe.Tokenizer(O.GPT4_SPLIT_PATTERN)
    tok.train(read_data("taylorswift.txt"), 512, conflict_resolution=cr, dedup=True, regions=True)
    tok.save(str(tmp_path / "tok.model"))
    assert (tmp_path / "tok.model").read_bytes() == read_golden("taylorswift_gpt4_%s_512.model" % name)
    sample = os.path.join(GOLDEN, "data", "sample.txt")
    for out, flags in (("plain.model", []), ("regions.model", ["--dedup", "--regions"])):
        r = subprocess.run([CLI, "--train"] + flags + ["-i", sample, "-m", str(tmp_path / out), "-c", name,
                                                        "--vocab-size", "400"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
    assert (tmp_path / "regions.model").read_bytes() == (tmp_path / "plain.model").read_bytes()
