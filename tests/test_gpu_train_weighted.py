"""Training on chunks with weights (mbpe_load_corpus_weighted, mbpe_load_corpus_endmask_weighted; the weighted 32-bit
loop of csrc/wide.hip) against the oracle on the EXPANDED corpus -- every chunk written out weights[c] times -- for
both tie-breaks: the chosen pair and its count at every step, and at the end the stream and chunk ends of an oracle
state on the unique text after the same merges, and the oracle's non-zero pairs on the expanded corpus."""
import numpy as np
import pytest

import mbpe
import oracle as O
import dedup_cases as C
from conftest import read_data
from test_gpu_wide import _word_corpus

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

MODES = [pytest.param(O.LEXICAL, id="lexical"), pytest.param(O.FIRST, id="first")]


@pytest.fixture(scope="module")
def tr():
    t = mbpe.Trainer(0)
    yield t
    t.close()


def _step_parity(tr, uniq, weights, full_chunks, vocab, mode, prior=None):
    """full_chunks: the corpus the weights stand for, in an order whose first occurrences are `uniq`'s order."""
    u_data, u_off = C.join(uniq)
    f_data, f_off = C.join(full_chunks)
    st = O.State(f_data, f_off, mode)
    tr.load_corpus_weighted(u_data, u_off, weights)
    tr.set_option("conflict_resolution", 1 if mode == O.LEXICAL else 0)
    n_prior = 0 if prior is None else len(prior)
    for k in range(n_prior):
        st.merge(int(prior[k][0]), int(prior[k][1]), 256 + k)
    tr.train_begin(vocab, prior)
    merges = [] if prior is None else [tuple(int(x) for x in p) for p in prior]
    for k in range(n_prior, vocab - 256):
        top = st.top()
        done = tr.train_steps(1)
        if top is None or (mode == O.FIRST and top[2] == 0):
            assert done == 0, "step %d: the oracle has no pair left" % k
            break
        assert done == 1, "step %d" % k
        m, c = tr.train_result()
        assert (int(m[k][0]), int(m[k][1]), int(c[k])) == top, "step %d" % k
        st.merge(top[0], top[1], 256 + k)
        merges.append((top[0], top[1]))
    # the stream is the unique text's, the table the expanded corpus's
    ust = O.State(u_data, u_off, mode)
    for k, (a, b) in enumerate(merges):
        ust.merge(a, b, 256 + k)
    want_toks, want_clen = ust.stream()
    toks, ends = tr.stream()
    assert np.array_equal(toks, want_toks)
    want_ends = np.zeros(len(want_toks), dtype=np.uint8)
    want_ends[np.cumsum(want_clen[want_clen > 0]).astype(np.int64) - 1] = 1
    assert np.array_equal(ends, want_ends)
    assert {k: v for k, v in tr.pairs_dict().items() if v} == {k: v for k, v in st.table_dict().items() if v}
    assert tr.decode_stream() == u_data.tobytes()
    ust.close()
    st.close()
    return merges


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("seed", range(4))
def test_dedup_of_small_alphabets(tr, seed, mode):
    # (a): runs, `a a a`, touching `abab`, candidates across the 1,024-token spans of the loop
    chunks = C.random_chunks(100 + seed, 3000, 12, 1 + seed)
    uniq, weights, _ = C.dedup(chunks)
    _step_parity(tr, uniq, weights, chunks, 256 + 60, mode)


@pytest.mark.parametrize("mode", MODES)
def test_weights_given_by_the_caller(tr, mode):
    # (b): 200 distinct chunks with weights of 1 .. 1,000; the expansion repeats every chunk in place
    rng = np.random.default_rng(7)
    uniq = list(dict.fromkeys(C.random_chunks(8, 260, 9, 4)))[:200]
    assert len(uniq) == 200
    weights = rng.integers(1, 1001, size=200).astype(np.uint32)
    full = [uniq[i] for i in np.repeat(np.arange(200), weights)]
    _step_parity(tr, uniq, weights, full, 256 + 50, mode)


@pytest.mark.parametrize("mode", MODES)
def test_zero_count_tail(tr, mode):
    # (c): the vocabulary outlasts the corpus: lexical fills the tail with zero-count pairs, `first` returns fewer merges
    data = read_data("small.txt")
    chunks = C.chunks_of(data, mbpe.presplit(O.GPT4_SPLIT_PATTERN, data))
    uniq, weights, _ = C.dedup(chunks)
    vocab = 256 + len(data)
    f_data, f_off = C.join(chunks)
    want_m, want_c = O.train(f_data, vocab, f_off, mode)
    u_data, u_off = C.join(uniq)
    m, c, _ = tr.train(u_data, vocab, u_off, conflict_resolution=1 if mode == O.LEXICAL else 0, weights=weights)
    assert m.tolist() == want_m.tolist() and c.tolist() == want_c.tolist()
    if mode == O.LEXICAL:
        assert len(m) == vocab - 256 and int(c[-1]) == 0
    else:
        assert 0 < len(m) < vocab - 256 and int(c[-1]) > 0


def test_limits(tr):
    # (d): counts up to 2^31 - 1 train -- on a stream of five tokens, which also proves that table headroom is bounded by
    # the stream's positions and not by a count
    data = np.frombuffer(b"abab?", dtype=np.uint8)
    off = np.array([0, 2, 5], dtype=np.uint64)
    for cr in (1, 0):
        m, c, _ = tr.train(data, 256 + 2, off, conflict_resolution=cr, weights=[1 << 30, (1 << 30) - 1])
        assert m.tolist() == [[97, 98], [256, 63]] and c.tolist() == [(1 << 31) - 1, (1 << 30) - 1]
    with pytest.raises(mbpe.MbpeError) as e:
        tr.train(data, 256 + 2, off, weights=[1 << 30, 1 << 30])
    assert e.value.code == mbpe.ERR_OVERFLOW
    for bad in ([0, 1], [1, 1 << 31], [1, (1 << 32) - 1]):
        with pytest.raises(mbpe.MbpeError) as e:
            tr.load_corpus_weighted(data, off, bad)
        assert e.value.code == mbpe.ERR_ARG


def test_limits_of_the_mask_variant(tr):
    dev = torch.device("cuda", 0)
    data = np.frombuffer(b"abab?", dtype=np.uint8)
    off = np.array([0, 2, 5], dtype=np.uint64)
    text = torch.from_numpy(np.concatenate([data, np.zeros(16, dtype=np.uint8)])).to(dev)
    mask = torch.from_numpy(C.end_mask(off, 5)).to(dev)

    def load(weights, on_device):
        if on_device:
            w = torch.from_numpy(np.asarray(weights, dtype=np.uint32).view(np.int32)).to(dev)
            tr.load_corpus_endmask_weighted(mask.data_ptr(), text_ptr=text.data_ptr(), n_bytes=5, weights_ptr=w.data_ptr(),
                                            n_weights=len(weights), keep=(text, mask, w))
        else:
            tr.load_corpus_endmask_weighted(mask.data_ptr(), weights=weights, data=data, keep=mask)

    for on_device in (False, True):
        for bad in ([0, 1], [1, 1 << 31], [1], [1, 2, 3]):      # a weight of 0, one of 2^31, too few, too many
            with pytest.raises(mbpe.MbpeError) as e:
                load(bad, on_device)
            assert e.value.code == mbpe.ERR_ARG, (bad, on_device)
        load([1 << 30, (1 << 30) - 1], on_device)
        tr.set_option("conflict_resolution", 1)
        tr.train_begin(258)
        assert tr.train_steps(2) == 2
        m, c = tr.train_result()
        assert m.tolist() == [[97, 98], [256, 63]] and c.tolist() == [(1 << 31) - 1, (1 << 30) - 1]
        with pytest.raises(mbpe.MbpeError) as e:
            tr.pair_count_u8()
        assert e.value.code == mbpe.ERR_STATE
        load([1 << 30, 1 << 30], on_device)
        with pytest.raises(mbpe.MbpeError) as e:
            tr.train_begin(258)
        assert e.value.code == mbpe.ERR_OVERFLOW


@pytest.mark.parametrize("mode", MODES)
def test_prior_merges_on_a_weighted_corpus(tr, mode):
    # (e): train to V0, continue to V: the same as training to V at once
    chunks = C.random_chunks(21, 3000, 10, 4)
    uniq, weights, _ = C.dedup(chunks)
    u_data, u_off = C.join(uniq)
    cr = 1 if mode == O.LEXICAL else 0
    whole_m, whole_c, _ = tr.train(u_data, 256 + 50, u_off, conflict_resolution=cr, weights=weights)
    f_data, f_off = C.join(chunks)
    want_m, want_c = O.train(f_data, 256 + 50, f_off, mode)
    assert whole_m.tolist() == want_m.tolist() and whole_c.tolist() == want_c.tolist()
    part_m, _, _ = tr.train(u_data, 256 + 20, u_off, conflict_resolution=cr, weights=weights)
    m, c, _ = tr.train(u_data, 256 + 50, u_off, conflict_resolution=cr, weights=weights, prior_merges=part_m)
    assert m.tolist() == whole_m.tolist()
    assert c[:20].tolist() == [-1] * 20 and c[20:].tolist() == whole_c[20:].tolist()
    _step_parity(tr, uniq, weights, chunks, 256 + 30, mode, prior=part_m)


def test_ids_beyond_16_bits(tr):
    # (f): the word corpus of test_gpu_wide.py, deduplicated: 4,200 unique words carry ids up to 67,999.  (Nearly all
    # of this test's time is the oracle's training on the expanded corpus, the reference test_gpu_wide.py takes too;
    # the 67,744 weighted merges on the device take seconds.)
    data, off = _word_corpus(78, 4200, 24, (6, 14))
    vocab = 68000
    want_m, want_c = O.train(data, vocab, off)
    chunks = C.chunks_of(data, off)
    uniq, weights, _ = C.dedup(chunks)
    assert len(uniq) == 4200 and min(weights) >= 6
    u_data, u_off = C.join(uniq)
    m, c, _ = tr.train(u_data, vocab, u_off, weights=weights)
    assert len(m) == vocab - 256 and int(m.max()) > 65535
    assert m.tolist() == want_m.tolist() and c.tolist() == want_c.tolist()
    assert tr.decode_stream() == u_data.tobytes()


def test_several_ranks_are_refused():
    # (g)
    data, off = C.join([b"abc", b"ab"])
    with mbpe.Trainer(0) as t:
        t.comm_init_external(0, 2)
        t.load_corpus_weighted(data, off, [3, 2])
        with pytest.raises(mbpe.MbpeError) as e:
            t.train_begin(260)
        assert e.value.code == mbpe.ERR_STATE
        with pytest.raises(mbpe.MbpeError) as e:
            t.train_begin(260, np.array([[97, 98]], dtype=np.uint32))
        assert e.value.code == mbpe.ERR_STATE


def test_the_dedupers_result_goes_in_without_a_host_round_trip(tr):
    dev = torch.device("cuda", 0)
    chunks = C.random_chunks(5, 5000, 8, 3)
    data, off = C.join(chunks)
    want_m, want_c = O.train(data, 256 + 40, off, O.FIRST)
    text = torch.from_numpy(np.concatenate([data, np.zeros(16, dtype=np.uint8)])).to(dev)
    mask = torch.from_numpy(C.end_mask(off, len(data))).to(dev)
    with mbpe.Deduper(0) as dd:
        nu, nb = dd.chunks_endmask(text.data_ptr(), len(data), mask.data_ptr())
        t_ptr, m_ptr, w_ptr, _ = dd.result()
        tr.load_corpus_endmask_weighted(m_ptr, text_ptr=t_ptr, n_bytes=nb, weights_ptr=w_ptr, n_weights=nu, keep=dd)
        tr.set_option("conflict_resolution", 0)
        tr.train_begin(256 + 40)
        tr.train_steps(40)
        m, c = tr.train_result()
    assert m.tolist() == want_m.tolist() and c.tolist() == want_c.tolist()
