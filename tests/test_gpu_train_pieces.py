"""Training on the table of mbpe.WordCount: WordCount.result() goes into Trainer.load_corpus_endmask_weighted in place,
and merges and counts must be the oracle's on the pieces' chunks laid end to end, for both tie-breaks -- with a repeated
piece, against the oracle on the written-out list."""
import pytest

import mbpe
import oracle as O
import dedup_cases as C
import wordcount_cases as W

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

MODES = [pytest.param(O.LEXICAL, id="lexical"), pytest.param(O.FIRST, id="first")]
VOCAB = 256 + 40


@pytest.fixture(scope="module")
def tr():
    t = mbpe.Trainer(0)
    yield t
    t.close()


def _pieces(seed):
    return W.cut_list(C.random_chunks(300 + seed, 900 + 200 * seed, 12, 1 + seed), 3)


# the oracle's training per (seed, repeats, mode): computed once, shared, never changed
_WANT = {}


def _want(seed, repeats, mode):
    key = (seed, repeats, mode)
    if key not in _WANT:
        written_out = [c for p, rep in zip(_pieces(seed), repeats) for c in p * rep]
        data, off = C.join(written_out)
        m, c = O.train(data, VOCAB, off, mode)
        _WANT[key] = (m.tolist(), c.tolist())
    return _WANT[key]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("repeats", [(1, 1, 1), (1, 3, 1)], ids=["plain", "repeat-3"])
@pytest.mark.parametrize("seed", range(4))
def test_training_on_the_accumulated_table(tr, seed, repeats, mode):
    want_m, want_c = _want(seed, repeats, mode)
    with mbpe.WordCount(0) as wc:
        for p, rep in zip(_pieces(seed), repeats):
            data, off = C.join(p)
            nu, nb = wc.add(data, off, repeat=rep)
        t_ptr, m_ptr, w_ptr, _ = wc.result()
        tr.load_corpus_endmask_weighted(m_ptr, text_ptr=t_ptr, n_bytes=nb, weights_ptr=w_ptr, n_weights=nu, keep=wc)
        tr.set_option("conflict_resolution", 1 if mode == O.LEXICAL else 0)
        tr.train_begin(VOCAB)
        tr.train_steps(VOCAB - 256)
        m, c = tr.train_result()
    assert m.tolist() == want_m and c.tolist() == want_c
