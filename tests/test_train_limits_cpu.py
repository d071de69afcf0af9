"""The Python restatement of the stopping rules (train_limits_cases.limited_bpe), checked without a GPU: against
dedup_cases.weighted_bpe with the limits off, against a walk of the C oracle's state under the rules, on the
properties the rules promise, and on the constructed cases whose results are known by hand."""
import numpy as np
import pytest

import oracle as O
import dedup_cases as C
import train_limits_cases as T

MODES = [pytest.param(False, id="lexical"), pytest.param(True, id="first")]


@pytest.mark.parametrize("first", MODES)
@pytest.mark.parametrize("seed", range(4))
def test_limits_off_is_weighted_bpe(seed, first):
    _, uniq, weights = T.random_inputs(seed)
    want = C.weighted_bpe(uniq, weights, 256 + 40, first)
    for trace in (True, False):
        m, c, _ = T.limited_bpe(uniq, weights, 256 + 40, first, trace=trace)
        assert (m, c) == want


def _oracle_walk(chunks, vocab, first, L, f):
    """The rules applied to the C oracle's own table and stream, step by step."""
    data, off = C.join(chunks)
    st = O.State(data, off, O.FIRST if first else O.LEXICAL)
    length = [1] * 256
    merges, counts = [], []
    for k in range(vocab - 256):
        tab = st.table_dict()
        if first:
            tab = {key: c for key, c in tab.items() if c > 0}      # (a recount holds no zero-count pair)
        elig = {key: c for key, c in tab.items() if L == 0 or length[key[0]] + length[key[1]] <= L}
        if not elig:
            break
        top = max(elig.values())
        if top < f or (first and top == 0):
            break
        tied = {key for key, c in elig.items() if c == top}
        if first:
            toks, clen = st.stream()
            ends = set(np.cumsum(clen[clen > 0]).astype(np.int64) - 1)
            win = next((int(toks[i]), int(toks[i + 1])) for i in range(len(toks) - 1)
                       if i not in ends and (int(toks[i]), int(toks[i + 1])) in tied)
        else:
            win = min(tied)
        merges.append(win)
        counts.append(top)
        length.append(length[win[0]] + length[win[1]])
        st.merge(win[0], win[1], 256 + k)
    st.close()
    return merges, counts


@pytest.mark.parametrize("first", MODES)
def test_against_a_walk_of_the_oracle(first):
    chunks = C.random_chunks(31, 400, 9, 3)
    uniq, weights, _ = C.dedup(chunks)
    for L, f in ((3, 0), (4, 6), (0, 9)):
        want = _oracle_walk(chunks, 256 + 25, first, L, f)
        m, c, tr = T.limited_bpe(uniq, weights, 256 + 25, first, L=L, f=f)
        assert (m, c) == want, (L, f)
        if L == 3:
            assert any(s["larger"] for s in tr)       # the limit did change choices
    # limits off: the oracle's own training
    data, off = C.join(chunks)
    om, oc = O.train(data, 256 + 25, off, O.FIRST if first else O.LEXICAL)
    m, c, _ = T.limited_bpe(uniq, weights, 256 + 25, first)
    assert [list(p) for p in m] == om.tolist() and c == oc.tolist()


@pytest.mark.parametrize("first", MODES)
@pytest.mark.parametrize("L", [2, 3, 5])
def test_no_new_token_is_longer_than_the_limit(L, first):
    _, uniq, weights = T.random_inputs(2)
    m, _, tr = T.limited_bpe(uniq, weights, 256 + 30, first, L=L)
    assert m and max(T.token_lengths(m)) <= L
    assert L == 5 or any(s["larger"] for s in tr)      # (30 merges of three symbols rarely reach five bytes)


@pytest.mark.parametrize("first", MODES)
def test_min_frequency_cuts_the_unlimited_result(first):
    _, uniq, weights = T.random_inputs(3)
    m0, c0, _ = T.limited_bpe(uniq, weights, 256 + 40, first)
    for f in (c0[0] + 1, c0[0], c0[15], c0[15] + 1, 1):
        cut = next((i for i, c in enumerate(c0) if c < f), len(c0))
        m, c, _ = T.limited_bpe(uniq, weights, 256 + 40, first, f=f)
        assert (m, c) == (m0[:cut], c0[:cut]), f


@pytest.mark.parametrize("first", MODES)
def test_continued_training_counts_prior_lengths(first):
    _, uniq, weights = T.random_inputs(3)
    prior, _, _ = T.limited_bpe(uniq, weights, 256 + 20, first)
    seqs = T.apply_merges(uniq, prior)
    m, c, _ = T.limited_bpe(uniq, weights, 256 + 40, first, L=2, start=(seqs, 20, prior))
    length = T.token_lengths(list(prior) + list(m))
    assert m and max(length[256 + 20:]) <= 2 and max(length[:256 + 20]) > 2      # the prior merges stay
    # with the limits off, continuing equals training at once
    whole, wc, _ = T.limited_bpe(uniq, weights, 256 + 40, first)
    m, c, _ = T.limited_bpe(uniq, weights, 256 + 40, first, start=(seqs, 20))
    assert (list(prior) + m, c) == (whole, wc[20:])
    with pytest.raises(ValueError):
        T.limited_bpe(uniq, weights, 256 + 40, first, L=3, start=(seqs, 20))


@pytest.mark.parametrize("case,event", [(T.CASE_A, "earlier_span"), (T.CASE_B, "smaller_key")])
def test_constructed_ties(case, event):
    chunks, L, vocab, lex_m, lex_c, first_m = case
    m, c, tr = T.limited_bpe(chunks, [1] * len(chunks), vocab, False, L=L)
    assert (m, c) == (lex_m, lex_c)
    assert any(s[event] for s in tr) and any(s["earlier_span"] for s in tr)
    m, c, tr = T.limited_bpe(chunks, [1] * len(chunks), vocab, True, L=L)
    assert (m, c) == (first_m, lex_c[:len(first_m)])
    assert any(s[event] for s in tr) and any(s["earlier_span"] for s in tr)


@pytest.mark.parametrize("first", MODES)
def test_constructed_min_frequency(first):
    chunks, weights, vocab, made = T.CASE_C
    for f, n in made.items():
        m, c, _ = T.limited_bpe(chunks, weights, vocab, first, f=f)
        assert (m, c) == ([(97, 98), (99, 100)][:n], [5, 4][:n]), f


@pytest.mark.parametrize("first", MODES)
def test_nothing_eligible(first):
    seqs = T.apply_merges([b"aaaa"], [(97, 97)])
    assert seqs == [[256, 256]]
    m, c, _ = T.limited_bpe([b"aaaa"], [1], 258, first, L=2, start=(seqs, 1, [(97, 97)]))
    assert (m, c) == ([], [])
    m, c, _ = T.limited_bpe([b"aaaa"], [1], 257 + 1, first, L=0, start=(seqs, 1, [(97, 97)]))
    assert (m[0], c[0]) == ((256, 256), 1)
