"""The stopping rules of a training ("min_frequency", "max_token_length"; the limited argmax of csrc/wide.hip) against
train_limits_cases.limited_bpe: the chosen pair and its count at every step, where the loop ends, and at the end the
stream, its chunk ends and the non-zero pairs -- on a corpus of unique chunks with weights and on the same corpus
written out and loaded without weights, which takes the same route."""
import functools

import numpy as np
import pytest

import mbpe
import dedup_cases as C
import train_limits_cases as T

pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

MODES = [pytest.param(False, id="lexical"), pytest.param(True, id="first")]
LOADS = [pytest.param(True, id="weighted"), pytest.param(False, id="unweighted")]


@pytest.fixture()
def tr():
    t = mbpe.Trainer(0)
    yield t
    t.close()


def _load(tr, chunks, weights, weighted, first, L, f):
    data, off = C.join(chunks)
    if weighted:
        tr.load_corpus_weighted(data, off, weights)
    else:
        tr.load_corpus(data, off)
    tr.set_option("conflict_resolution", 0 if first else 1)
    tr.set_option("max_token_length", L)
    tr.set_option("min_frequency", f)


def _check_end(tr, chunks, weights, merges):
    """stream, chunk ends and non-zero pairs after `merges` (prior ones included)"""
    seqs = T.apply_merges(chunks, merges)
    toks, ends = tr.stream()
    assert toks.tolist() == [t for s in seqs for t in s]
    want_ends = np.zeros(len(toks), dtype=np.uint8)
    want_ends[np.cumsum([len(s) for s in seqs if s]) - 1] = 1
    assert np.array_equal(ends, want_ends)
    want = {}
    for s, w in zip(seqs, weights):
        for i in range(len(s) - 1):
            want[(s[i], s[i + 1])] = want.get((s[i], s[i + 1]), 0) + int(w)
    assert {k: v for k, v in tr.pairs_dict().items() if v} == want


def _step_parity(tr, chunks, weights, vocab, first, L, f, weighted, want, prior=None):
    """want: limited_bpe's (merges, counts) for this corpus -- from its unique chunks with counts or written out, the
    result is the same"""
    want_m, want_c = want
    n_prior = 0 if prior is None else len(prior)
    _load(tr, chunks, weights, weighted, first, L, f)
    tr.train_begin(vocab, None if prior is None else np.asarray(prior, dtype=np.uint32))
    for k, (pair, cnt) in enumerate(zip(want_m, want_c)):
        assert tr.train_steps(1) == 1, "step %d" % k
        m, c = tr.train_result()
        assert (tuple(int(x) for x in m[n_prior + k]), int(c[n_prior + k])) == (pair, cnt), "step %d" % k
    if n_prior + len(want_m) < vocab - 256:          # the training ended early: no further step, now or later
        assert tr.train_steps(1) == 0 and tr.train_steps(5) == 0
    m, _ = tr.train_result()
    assert len(m) == n_prior + len(want_m)
    _check_end(tr, chunks, weights, ([] if prior is None else list(prior)) + list(want_m))
    # all at once: groups of 16 merges per launch sequence, and the host's zero-count fill (lexical)
    tr.train_begin(vocab, None if prior is None else np.asarray(prior, dtype=np.uint32))
    assert tr.train_steps(vocab - 256) == len(want_m)
    m, c = tr.train_result()
    assert [tuple(p) for p in m[n_prior:].tolist()] == list(want_m) and c[n_prior:].tolist() == list(want_c)
    assert tr.train_steps(3) == 0 or n_prior + len(want_m) == vocab - 256


@functools.lru_cache(maxsize=None)
def _random_want(seed, first, L):
    _, uniq, weights = T.random_inputs(seed)
    m, c, trace = T.limited_bpe(uniq, weights, 256 + 30, first, L=L)
    return (m, c), sum(s["larger"] for s in trace)


@pytest.mark.parametrize("weighted", LOADS)
@pytest.mark.parametrize("first", MODES)
@pytest.mark.parametrize("L", [2, 3, 5])
@pytest.mark.parametrize("seed", range(4))
def test_random_chunks(tr, seed, L, first, weighted):
    chunks, uniq, weights = T.random_inputs(seed)
    want, n_larger = _random_want(seed, first, L)
    if seed and L == 2:
        assert n_larger > 0          # an ineligible pair led the table: the limit decided
    if seed == 0:                    # one letter: lexical reaches the eligible zero-count pairs, `first` ends early
        assert (len(want[0]) <= 4) if first else (len(want[0]) == 30 and want[1][-1] == 0)
    if weighted:
        _step_parity(tr, uniq, weights, 256 + 30, first, L, 0, True, want)
    else:
        _step_parity(tr, chunks, [1] * len(chunks), 256 + 30, first, L, 0, False, want)


@pytest.mark.parametrize("weighted", LOADS)
@pytest.mark.parametrize("first", MODES)
@pytest.mark.parametrize("case,event", [pytest.param(T.CASE_A, "earlier_span", id="A"),
                                        pytest.param(T.CASE_B, "smaller_key", id="B")])
def test_constructed_ties(tr, case, event, first, weighted):
    chunks, L, vocab, lex_m, lex_c, first_m = case
    weights = [1] * len(chunks)
    m, c, trace = T.limited_bpe(chunks, weights, vocab, first, L=L)
    assert (m, c) == ((first_m, lex_c[:len(first_m)]) if first else (lex_m, lex_c))
    assert any(s[event] for s in trace) and any(s["earlier_span"] for s in trace)
    _step_parity(tr, chunks, weights, vocab, first, L, 0, weighted, (m, c))


@pytest.mark.parametrize("first", MODES)
def test_min_frequency(tr, first):
    # a count equal to min_frequency trains
    chunks, weights, vocab, made = T.CASE_C
    for f, n in made.items():
        want = ([(97, 98), (99, 100)][:n], [5, 4][:n])
        assert T.limited_bpe(chunks, weights, vocab, first, f=f)[:2] == want
        _step_parity(tr, chunks, weights, vocab, first, 0, f, True, want)
        full = [chunks[0]] * 5 + [chunks[1]] * 4
        _step_parity(tr, full, [1] * 9, vocab, first, 0, f, False, want)


@pytest.mark.parametrize("weighted", LOADS)
@pytest.mark.parametrize("first", MODES)
def test_nothing_eligible(tr, first, weighted):
    prior = [(97, 97)]
    _load(tr, [b"aaaa"], [1], weighted, first, 2, 0)
    tr.train_begin(258, np.asarray(prior, dtype=np.uint32))
    assert tr.train_steps(1) == 0 and tr.train_steps(2) == 0
    m, c = tr.train_result()
    assert m.tolist() == [[97, 97]] and c.tolist() == [-1]
    assert tr.stream()[0].tolist() == [256, 256]
    # without the limit the same prior merges (256, 256)
    _load(tr, [b"aaaa"], [1], weighted, first, 0, 0)
    tr.train_begin(258, np.asarray(prior, dtype=np.uint32))
    assert tr.train_steps(1) == 1
    m, c = tr.train_result()
    assert m.tolist() == [[97, 97], [256, 256]] and c.tolist() == [-1, 1]


@pytest.mark.parametrize("weighted", LOADS)
@pytest.mark.parametrize("first", MODES)
def test_continued(tr, first, weighted):
    chunks, uniq, weights = T.random_inputs(3)
    prior, _, _ = T.limited_bpe(uniq, weights, 256 + 20, first)
    want = T.limited_bpe(uniq, weights, 256 + 40, first, L=3, start=(T.apply_merges(uniq, prior), 20, prior))[:2]
    assert want[0] and max(T.token_lengths(prior + want[0])[256 + 20:]) <= 3
    if weighted:
        _step_parity(tr, uniq, weights, 256 + 40, first, 3, 0, True, want, prior=prior)
    else:
        _step_parity(tr, chunks, [1] * len(chunks), 256 + 40, first, 3, 0, False, want, prior=prior)


@pytest.mark.parametrize("first", MODES)
def test_table_growth(tr, first):
    # (16 symbols: the table starts small, at 8,192 slots, and takes ~9,000 pairs; from merge ~520 on the unlimited
    #  training would choose pairs of four bytes)
    chunks = C.random_chunks(7, 3000, 12, 16)
    uniq, weights, _ = C.dedup(chunks)
    want_m, want_c, _ = T.limited_bpe(uniq, weights, 256 + 600, first, L=3, f=2, trace=False)
    assert len(want_m) > 300 and want_m != T.limited_bpe(uniq, weights, 256 + 600, first, f=2, trace=False)[0]
    _load(tr, uniq, weights, True, first, 3, 2)
    tr.train_begin(256 + 600)
    assert tr.train_steps(600) == len(want_m)
    assert tr.stats()["n_table_grows"] > 0
    m, c = tr.train_result()
    assert [tuple(p) for p in m.tolist()] == want_m and c.tolist() == want_c
    assert max(T.token_lengths(want_m)) <= 3
    _check_end(tr, uniq, weights, want_m)


def test_errors(tr):
    for name, bad in (("max_token_length", 1), ("max_token_length", -1), ("max_token_length", 1 << 31),
                      ("min_frequency", -1), ("min_frequency", 1 << 31)):
        with pytest.raises(mbpe.MbpeError) as e:
            tr.set_option(name, bad)
        assert e.value.code == mbpe.ERR_ARG, (name, bad)
    tr.set_option("max_token_length", (1 << 31) - 1)
    tr.set_option("min_frequency", (1 << 31) - 1)
    data = np.frombuffer(b"abcabcabd" * 50, dtype=np.uint8)
    for L, f in ((4, 0), (0, 2)):
        tr.load_corpus(data)
        tr.set_option("max_token_length", L)
        tr.set_option("min_frequency", f)
        tr.set_option("force_exchange", 1)
        with pytest.raises(mbpe.MbpeError) as e:
            tr.train_begin(512)
        assert e.value.code == mbpe.ERR_STATE
        tr.set_option("force_exchange", 0)
        with pytest.raises(mbpe.MbpeError) as e:
            tr.train_begin((1 << 24) + 1)
        assert e.value.code == mbpe.ERR_VOCAB
        tr.train_begin(512)
        with pytest.raises(mbpe.MbpeError) as e:      # the limited training runs on 32-bit tokens: no dense table
            tr.table_device()
        assert e.value.code == mbpe.ERR_STATE
    # both back to 0: the slot route again
    tr.set_option("max_token_length", 0)
    tr.set_option("min_frequency", 0)
    tr.train_begin(512)
    assert tr.train_steps(4) == 4
    ptr, _ = tr.table_device()
    assert ptr
