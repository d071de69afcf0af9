"""The cases of tests/weighted_limit_cases.py, without a GPU: that each is what its name says -- the expect flag, the
margins to the limits, the token, share and span counts, the distinct pairs of a share -- decided by the reference
alone, in Python integers; and the reference() wrapper itself against the oracle on the expanded corpus, final sequences
and table included, with the weights divided down to at most 50."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle as O
import dedup_cases as C
import weighted_limit_cases as K

L = K.L
MODES = [pytest.param(False, id="lexical"), pytest.param(True, id="first")]


def _well_formed(chunks, weights):
    assert len(chunks) == len(weights) and all(len(c) > 0 for c in chunks)
    assert all(isinstance(w, int) and 0 < w < L for w in weights)
    assert all(0 not in c for c in chunks)                 # (no chunk the NUL rule could make inert)
    assert K.n_tokens(chunks) < 20000


def test_the_cases_module_needs_no_torch():
    here = os.path.dirname(os.path.abspath(__file__))
    code = "import sys; sys.path.insert(0, %r); import weighted_limit_cases; assert 'torch' not in sys.modules" % here
    subprocess.check_call([sys.executable, "-c", code])


@pytest.mark.parametrize("variant", ["a", "b"])
def test_sum_beyond_2_32(variant):
    chunks, weights, vocab, expect = K.sum_beyond_2_32(variant)
    _well_formed(chunks, weights)
    assert expect == "trains" and vocab == 256 + 40
    assert len(set(chunks)) == len(chunks) and 2200 < len(chunks) < 2400
    n = K.n_tokens(chunks)
    assert 15000 < n < 17000 and len(K.shares(n)) == 4 and K.n_spans(chunks) >= 15
    counts = K.initial_counts(chunks, weights)
    top, total = max(counts.values()), sum(counts.values())
    assert L - L // 64 < top < L
    assert total > 100 << 32                                # every 32-bit sum of the positions wraps many times
    if variant == "a":
        assert len(set(weights)) == 1
        assert top == 2147483637 and total >> 32 == 174
    else:
        assert len(set(weights)) > len(weights) // 2


def test_many_distinct_pairs():
    chunks, weights, vocab, expect = K.many_distinct_pairs()
    _well_formed(chunks, weights)
    assert expect == "trains"
    assert len({b for c in chunks for b in c}) == 64
    assert len(K.distinct_pairs(chunks, 0, K.SHARE)) > 2048
    for lo, hi in K.shares(K.n_tokens(chunks)):             # every workgroup overflows its cache
        assert len(K.distinct_pairs(chunks, lo, hi)) > 2 * K.LDS_SLOTS - 200
    assert len(set(weights)) > len(weights) - 3 and sorted(weights)[len(weights) // 2] > 1 << 24
    top = max(K.initial_counts(chunks, weights).values())
    assert L - L // 64 < top < L


@pytest.mark.parametrize("layout", K.LAYOUTS)
@pytest.mark.parametrize("c", K.LADDER_COUNTS)
def test_ladder(c, layout):
    chunks, weights, vocab, expect = K.ladder(c, layout)
    _well_formed(chunks, weights)
    pair = K.heavy_pair(layout)
    assert (pair[0] == pair[1]) == (layout == "in_run") and max(pair) < min(b for ch in chunks for b in ch if b not in pair)
    counts = K.initial_counts(chunks, weights)
    assert counts[pair] == c
    assert max(v for k, v in counts.items() if k != pair) < 1 << 30
    assert expect == ("trains" if c in (L - 2, L - 1) else "overflow")
    holders = [(ch, w) for ch, w in zip(chunks, weights) if K.positions_of([ch], pair)]
    assert len(holders) >= 4 and all(w < L for _, w in holders)
    pos = K.positions_of(chunks, pair)
    n = K.n_tokens(chunks)
    sh = K.shares(n)
    in_share = sorted({i for p in pos for i, (lo, hi) in enumerate(sh) if lo <= p < hi})
    assert pos[0] > 100                                       # not first in the stream
    if layout in ("one_share", "in_chunk", "in_run"):
        assert pos[-1] < K.SHARE and in_share == [0] and len(sh) == 1
        assert pos[0] < K.SPAN < pos[-1]                      # ... but in two spans of the merge
    if layout in ("in_chunk", "in_run"):
        assert sum(len(K.positions_of([ch], pair)) >= 2 for ch, _ in holders) >= 3
    if layout == "across_shares":
        assert n >= 3 * K.SHARE and len(in_share) >= 3 and len({p // K.SHARE for p in pos}) >= 3
        assert all(w == 1 for ch, w in zip(chunks, weights) if not K.positions_of([ch], pair))
    if layout == "direct":
        assert len(K.distinct_pairs(chunks, 0, K.SHARE)) > 2048
        for i in in_share:                                    # the cache is long full where the pair first shows
            lo, hi = sh[i]
            first = min(p for p in pos if lo <= p < hi)
            assert len(K.distinct_pairs(chunks, lo, first)) > K.LDS_SLOTS + 512
            # ... and each slot this pair may take is gone four rounds of the workgroup's 256 threads before that
            assert K.cache_is_full_for(chunks, pair, lo, first - 4 * 256)


def test_ties_at_the_top():
    chunks, weights, vocab, expect = K.ties_at_the_top()
    _well_formed(chunks, weights)
    assert expect == "trains"
    counts = K.initial_counts(chunks, weights)
    assert sorted(K.TIED) == K.TIED
    assert [counts[p] for p in K.TIED] == [L - 1] * 3 and max(counts.values()) == L - 1
    assert sorted(v for v in counts.values() if v == L - 1) == [L - 1] * 3
    first_at = [K.positions_of(chunks, p)[0] for p in K.TIED]
    assert first_at[2] == 0 and first_at[1] == K.SPAN and first_at[0] > first_at[1]
    assert K.trained("ties_at_the_top", False).merges[:3] == K.TIED              # by key
    assert K.trained("ties_at_the_top", True).merges[:3] == K.TIED[::-1]         # by position
    assert K.trained("ties_at_the_top", False).counts[:3] == [L - 1] * 3 == K.trained("ties_at_the_top", True).counts[:3]


@pytest.mark.parametrize("first_mode", MODES)
@pytest.mark.parametrize("name", list(K.TRAINS))
def test_chosen_counts_stay_below_the_limit(name, first_mode):
    chunks, weights, vocab, expect = K.TRAINS[name]()
    assert expect == "trains"
    ref = K.trained(name, first_mode)
    assert len(ref.merges) == vocab - 256 == len(ref.counts)
    assert ref.counts[0] == max(K.initial_counts(chunks, weights).values())
    assert all(0 < c < L for c in ref.counts)
    assert all(x >= y for x, y in zip(ref.counts, ref.counts[1:]))
    assert max(ref.table.values()) <= ref.counts[-1]
    assert O.decode([t for s in ref.seqs for t in s], ref.merges) == b"".join(chunks)


@pytest.mark.parametrize("first_mode", MODES)
def test_prior_then_limits(first_mode):
    chunks, weights, vocab, expect = K.prior_then_limits()
    prior, ref = K.trained_from_prior(first_mode)
    whole = K.trained("sum_beyond_2_32-b", first_mode)
    assert len(prior) == K.N_PRIOR and prior == whole.merges[:K.N_PRIOR]
    replayed = K.replay(chunks, prior)
    assert max(t for s in replayed for t in s) == 255 + K.N_PRIOR
    top = max(K.recount(replayed, weights).values())
    assert L - L // 8 < top < L and sum(K.recount(replayed, weights).values()) > 100 << 32
    assert ref.merges == whole.merges[K.N_PRIOR:] and ref.counts == whole.counts[K.N_PRIOR:]
    assert ref.seqs == whole.seqs and ref.table == whole.table


def _smallest(n):
    return sorted(K.TRAINS, key=lambda name: K.n_tokens(K.TRAINS[name]()[0]))[:n]


@pytest.mark.parametrize("mode", [O.LEXICAL, O.FIRST], ids=["lexical", "first"])
@pytest.mark.parametrize("name", list(dict.fromkeys(_smallest(3) + ["ties_at_the_top"])))
def test_reference_against_the_oracle_on_the_expanded_corpus(name, mode):
    chunks, weights, vocab, _ = K.TRAINS[name]()
    w = [max(1, x * 50 // max(weights)) for x in weights]
    assert max(w) == 50
    full = [c for c, k in zip(chunks, w) for _ in range(k)]
    f_data, f_off = C.join(full)
    u_data, u_off = C.join(chunks)
    want_m, want_c = O.train(f_data, vocab, f_off, mode)
    ref = K.reference(chunks, w, vocab, mode == O.FIRST)
    assert ref.merges == [tuple(x) for x in want_m.tolist()] and ref.counts == want_c.tolist()
    # the sequences are the unique text's, the table the expanded corpus's
    st, ust = O.State(f_data, f_off, mode), O.State(u_data, u_off, mode)
    for k, (a, b) in enumerate(ref.merges):
        st.merge(a, b, 256 + k)
        ust.merge(a, b, 256 + k)
    toks, clen = ust.stream()
    assert [len(s) for s in ref.seqs] == clen.tolist()
    assert np.array_equal(K.stream_of(ref.seqs)[0], toks)
    assert ref.table == {k: v for k, v in st.table_dict().items() if v}
    st.close()
    ust.close()
    assert K.initial_counts(chunks, w) == {k: v for k, v in O.State(f_data, f_off, mode).table_dict().items() if v}
    # continued from its own first merges: the rest of the same training
    for n_prior in (1, 5):
        cont = K.reference(chunks, w, vocab, mode == O.FIRST, prior=ref.merges[:n_prior])
        assert cont.merges == ref.merges[n_prior:] and cont.counts == ref.counts[n_prior:]
        assert cont.seqs == ref.seqs and cont.table == ref.table
