"""The weighted 32-bit training loop (csrc/wide.hip under WideRun::begin_from, csrc/wide_run.cpp) at its limits, on the cases of
tests/weighted_limit_cases.py: a corpus whose weighted positions add up to far more than 2^32 trains, step for step, to
what the reference in Python integers gives -- pair and count at every step, then the stream, the chunk ends, the
non-zero table and the decoded text -- and a pair whose true count is 2^31 or more, up to beyond 2^33 and wherever its
occurrences lie, is refused with ERR_OVERFLOW, after which the same trainer trains the next corpus exactly."""
import numpy as np
import pytest

import mbpe
import dedup_cases as C
import weighted_limit_cases as K

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

L = K.L
MODES = [pytest.param(False, id="lexical"), pytest.param(True, id="first")]


@pytest.fixture(scope="module")
def tr():
    # one trainer for the whole module: what a refused training leaves behind is part of what is tested
    t = mbpe.Trainer(0)
    yield t
    t.close()


def _load(tr, chunks, weights):
    data, off = C.join(chunks)
    tr.load_corpus_weighted(data, off, weights)


def _step_parity(tr, chunks, vocab, first_mode, ref, prior=None):
    """The corpus is loaded; ref: the Reference of the merges from len(prior) on."""
    tr.set_option("conflict_resolution", 0 if first_mode else 1)
    n_prior = 0 if prior is None else len(prior)
    assert len(ref.merges) == vocab - 256 - n_prior
    tr.train_begin(vocab, None if prior is None else np.array(prior, dtype=np.uint32))
    for j, (pair, count) in enumerate(zip(ref.merges, ref.counts)):
        k = n_prior + j
        assert tr.train_steps(1) == 1, "step %d" % k
        m, c = tr.train_result()
        assert (int(m[k][0]), int(m[k][1]), int(c[k])) == (pair[0], pair[1], count), "step %d" % k
    if prior is not None:
        assert [tuple(x) for x in m[:n_prior].tolist()] == list(prior)
    want_toks, want_ends = K.stream_of(ref.seqs)
    toks, ends = tr.stream()
    assert np.array_equal(toks, want_toks)
    assert np.array_equal(ends, want_ends)
    assert {k: v for k, v in tr.pairs_dict().items() if v} == ref.table
    assert tr.decode_stream() == b"".join(chunks)


@pytest.mark.parametrize("first_mode", MODES)
@pytest.mark.parametrize("name", list(K.TRAINS))
def test_cases_that_train(tr, name, first_mode):
    chunks, weights, vocab, expect = K.TRAINS[name]()
    assert expect == "trains"
    _load(tr, chunks, weights)
    _step_parity(tr, chunks, vocab, first_mode, K.trained(name, first_mode))


@pytest.mark.parametrize("first_mode", MODES)
def test_prior_then_limits(tr, first_mode):
    chunks, weights, vocab, _ = K.prior_then_limits()
    prior, ref = K.trained_from_prior(first_mode)
    _load(tr, chunks, weights)
    _step_parity(tr, chunks, vocab, first_mode, ref, prior=prior)


@pytest.mark.parametrize("first_mode", MODES)
def test_text_mask_and_weights_on_the_device(tr, first_mode):
    dev = torch.device("cuda", 0)
    chunks, weights, vocab, _ = K.sum_beyond_2_32("b")
    data, off = C.join(chunks)
    text = torch.from_numpy(np.concatenate([data, np.zeros(16, dtype=np.uint8)])).to(dev)
    mask = torch.from_numpy(C.end_mask(off, len(data))).to(dev)
    w = torch.from_numpy(np.asarray(weights, dtype=np.uint32).view(np.int32)).to(dev)
    tr.load_corpus_endmask_weighted(mask.data_ptr(), text_ptr=text.data_ptr(), n_bytes=len(data), weights_ptr=w.data_ptr(),
                                    n_weights=len(weights), keep=(text, mask, w))
    _step_parity(tr, chunks, vocab, first_mode, K.trained("sum_beyond_2_32-b", first_mode))


@pytest.mark.parametrize("first_mode", MODES)
@pytest.mark.parametrize("c,layout", K.OVERFLOWS, ids=["%s-L%+d" % (layout, c - L) for c, layout in K.OVERFLOWS])
def test_a_count_of_2_31_or_more_is_refused(tr, c, layout, first_mode):
    chunks, weights, vocab, expect = K.ladder(c, layout)
    assert expect == "overflow"
    _load(tr, chunks, weights)
    tr.set_option("conflict_resolution", 0 if first_mode else 1)
    with pytest.raises(mbpe.MbpeError) as e:
        tr.train_begin(vocab)
    assert e.value.code == mbpe.ERR_OVERFLOW
    # right after it, on the same trainer: the same layout with one occurrence fewer than the limit, exactly
    chunks, weights, vocab, expect = K.ladder(L - 1, layout)
    _load(tr, chunks, weights)
    _step_parity(tr, chunks, vocab, first_mode, K.trained("ladder-%s-L-1" % layout, first_mode))


def _chunk_at_token(chunks, token):
    pos = 0
    for i, c in enumerate(chunks):
        if pos + len(c) > token:
            return i
        pos += len(c)
    raise AssertionError(token)


@pytest.mark.parametrize("bad", [0, L], ids=["0", "L"])
@pytest.mark.parametrize("where", ["last", "middle"])
def test_a_bad_weight_inside_a_long_corpus(tr, where, bad):
    dev = torch.device("cuda", 0)
    chunks, good, vocab, _ = K.ladder(L - 1, "across_shares")
    assert K.n_tokens(chunks) >= 12000
    at = len(chunks) - 1 if where == "last" else _chunk_at_token(chunks, 6 * K.SPAN + 500)
    weights = list(good)
    weights[at] = bad
    data, off = C.join(chunks)
    text = torch.from_numpy(np.concatenate([data, np.zeros(16, dtype=np.uint8)])).to(dev)
    mask = torch.from_numpy(C.end_mask(off, len(data))).to(dev)
    w = torch.from_numpy(np.asarray(weights, dtype=np.uint32).view(np.int32)).to(dev)
    with pytest.raises(mbpe.MbpeError) as e:
        tr.load_corpus_weighted(data, off, weights)
    assert e.value.code == mbpe.ERR_ARG
    with pytest.raises(mbpe.MbpeError) as e:
        tr.load_corpus_endmask_weighted(mask.data_ptr(), weights=weights, data=data, keep=mask)
    assert e.value.code == mbpe.ERR_ARG
    with pytest.raises(mbpe.MbpeError) as e:
        tr.load_corpus_endmask_weighted(mask.data_ptr(), text_ptr=text.data_ptr(), n_bytes=len(data),
                                        weights_ptr=w.data_ptr(), n_weights=len(weights), keep=(text, mask, w))
    assert e.value.code == mbpe.ERR_ARG
    # nothing is loaded after a refusal, and the good weights train on the same trainer
    with pytest.raises(mbpe.MbpeError) as e:
        tr.train_begin(vocab)
    assert e.value.code == mbpe.ERR_STATE
    w = torch.from_numpy(np.asarray(good, dtype=np.uint32).view(np.int32)).to(dev)
    tr.load_corpus_endmask_weighted(mask.data_ptr(), text_ptr=text.data_ptr(), n_bytes=len(data),
                                    weights_ptr=w.data_ptr(), n_weights=len(good), keep=(text, mask, w))
    _step_parity(tr, chunks, vocab, True, K.trained("ladder-across_shares-L-1", True))


@pytest.mark.parametrize("first_mode", MODES)
def test_train_in_one_call(tr, first_mode):
    chunks, weights, vocab, _ = K.sum_beyond_2_32("a")
    ref = K.trained("sum_beyond_2_32-a", first_mode)
    data, off = C.join(chunks)
    m, c, _ = tr.train(data, vocab, off, conflict_resolution=0 if first_mode else 1, weights=weights)
    assert [tuple(x) for x in m.tolist()] == ref.merges and c.tolist() == ref.counts
