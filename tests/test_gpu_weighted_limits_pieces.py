"""The 2^31 limit of a pair count where the weights come from mbpe.WordCount and from the pieces session of the
Tokenizer (train_from_iterator, `--input-list`): repeats that bring chunk weights to between 2^30 and 2^31 - 1 train to
what the reference of tests/weighted_limit_cases.py gives; a table whose every weight is fine while a pair shared by two
chunks reaches 2^31 is refused by the training with ERR_OVERFLOW, and then the tokenizer is what it was before."""
import os
import re
import subprocess

import numpy as np
import pytest

import mbpe
import oracle as O
import dedup_cases as C
import wordcount_cases as W
import weighted_limit_cases as K
from conftest import ROOT
from test_gpu_wordcount import _equal

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

L = K.L
MODES = [pytest.param(False, id="lexical"), pytest.param(True, id="first")]
SPLITS = [pytest.param(False, id="host-split"), pytest.param(True, id="device-split")]
CLI = os.path.join(ROOT, "minbpe-cc_amd", "minbpe-cc")


@pytest.fixture(scope="module")
def dev():
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def tr():
    t = mbpe.Trainer(0)
    yield t
    t.close()


def _disjoint_chunks(n):
    """n chunks of 2 .. 4 bytes, no byte value in two of them: no pair is shared, a pair's count is its chunk's weight."""
    out, sym = [], 1
    for i in range(n):
        k = 2 + i % 3
        out.append(bytes(range(sym, sym + k)))
        sym += k
    assert sym <= 256
    return out


def _load_table(tr, wc):
    t_ptr, m_ptr, w_ptr, _ = wc.result()
    tr.load_corpus_endmask_weighted(m_ptr, text_ptr=t_ptr, n_bytes=wc.n_unique_bytes, weights_ptr=w_ptr,
                                    n_weights=wc.n_unique, keep=wc)


def _step_parity(tr, vocab, first_mode, ref, text):
    tr.set_option("conflict_resolution", 0 if first_mode else 1)
    tr.train_begin(vocab)
    for k, (pair, count) in enumerate(zip(ref.merges, ref.counts)):
        assert tr.train_steps(1) == 1, "step %d" % k
        m, c = tr.train_result()
        assert (int(m[k][0]), int(m[k][1]), int(c[k])) == (pair[0], pair[1], count), "step %d" % k
    want_toks, want_ends = K.stream_of(ref.seqs)
    toks, ends = tr.stream()
    assert np.array_equal(toks, want_toks) and np.array_equal(ends, want_ends)
    assert {k: v for k, v in tr.pairs_dict().items() if v} == ref.table
    assert tr.decode_stream() == text


@pytest.mark.parametrize("first_mode", MODES)
def test_wordcount_weights_between_2_30_and_2_31(tr, dev, first_mode):
    chunks = _disjoint_chunks(60)
    pieces = [(chunks, 1 << 29), (chunks[::2] + chunks[::3], 1 << 28), (chunks[::-1], (1 << 29) + 7)]
    acc = W.Accumulator()
    with mbpe.WordCount(0) as wc:
        for p, rep in pieces:
            data, off = C.join(p)
            wc.add(data, off, repeat=rep)
            acc.add(p, rep)
        uniq, weights, _ = acc.result()
        assert uniq == chunks and len(set(weights)) == 3 and all(1 << 30 < w < L for w in weights)
        assert acc.n_chunks_total > 16 << 32
        _equal(wc, acc.result(), acc.n_chunks_total, dev)
        assert wc.stats() == {"n_pieces": 3, "n_chunks_total": acc.n_chunks_total, "n_unique": len(uniq),
                              "n_unique_bytes": K.n_tokens(uniq)}
        vocab = 256 + 30
        ref = K.reference(uniq, weights, vocab, first_mode)
        assert len(ref.merges) == 30 and max(ref.counts) < L and ref.counts[0] == max(weights)
        _load_table(tr, wc)
        _step_parity(tr, vocab, first_mode, ref, b"".join(uniq))


@pytest.mark.parametrize("first_mode", MODES)
def test_a_table_that_is_fine_while_a_pair_is_not(tr, first_mode):
    with mbpe.WordCount(0) as wc:
        wc.add(*C.join([b"abc", b"xy"]), repeat=1 << 30)
        wc.add(*C.join([b"abd"]), repeat=1 << 30)
        text, off, w, _ = wc.get()
        assert text == b"abcxyabd" and off.tolist() == [0, 3, 5, 8] and w.tolist() == [1 << 30] * 3
        assert K.initial_counts([b"abc", b"xy", b"abd"], w.tolist())[(97, 98)] == L
        _load_table(tr, wc)
        tr.set_option("conflict_resolution", 0 if first_mode else 1)
        with pytest.raises(mbpe.MbpeError) as e:
            tr.train_begin(256 + 4)
        assert e.value.code == mbpe.ERR_OVERFLOW
        # one occurrence fewer, on the same trainer: (a, b) occurs 2^31 - 1 times
        wc.reset()
        wc.add(*C.join([b"abc", b"xy"]), repeat=(1 << 30) - 1)
        wc.add(*C.join([b"abd"]), repeat=1 << 30)
        uniq, weights = [b"abc", b"xy", b"abd"], [(1 << 30) - 1, (1 << 30) - 1, 1 << 30]
        assert wc.get()[2].tolist() == weights
        ref = K.reference(uniq, weights, 256 + 4, first_mode)
        assert ref.merges[0] == (97, 98) and ref.counts[0] == L - 1
        _load_table(tr, wc)
        _step_parity(tr, 256 + 4, first_mode, ref, b"abcxyabd")


# ---- the Tokenizer's pieces session --------------------------------------------------------------------------------------
# gpt4 split: `abc`, ` de` / `abd`, ` fg` / the words of the third text; (a, b) is shared by the first two texts' first
# chunks and by nothing else, so its count is the sum of their repeats
TEXTS = [b"abc de", b"abd fg", b"the cat sat on the mat"]
FINE = [(1 << 30) - 1, 1 << 30, 3]
TOO_MANY = [1 << 30, 1 << 30, 3]
VOCAB = 256 + 12
PROBE = b"abc abd the cat de fg mat"


def _reference(repeats, first_mode, prior=None):
    acc = W.Accumulator()
    for t, rep in zip(TEXTS, repeats):
        acc.add(C.chunks_of(t, mbpe.presplit(O.GPT4_SPLIT_PATTERN, t)), rep)
    uniq, weights, _ = acc.result()
    assert max(weights) < L                                  # the table itself is fine either way
    return K.initial_counts(uniq, weights), K.reference(uniq, weights, VOCAB, first_mode, prior=prior)


def _model(tok, tmp_path):
    path = str(tmp_path / "probe.model")
    tok.save(path)
    with open(path, "rb") as f:
        return f.read()


def _snapshot(tok, tmp_path):
    return tok.merges().tolist(), _model(tok, tmp_path), tok.encode(PROBE).tolist(), tok.encode(PROBE, device=0).tolist()


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("first_mode", MODES)
def test_train_from_iterator_at_the_limit(tmp_path, first_mode, split):
    cr = 0 if first_mode else 1
    counts, ref = _reference(FINE, first_mode)
    assert counts[(97, 98)] == L - 1 == max(counts.values()) and len(ref.merges) == VOCAB - 256
    assert _reference(TOO_MANY, first_mode)[0][(97, 98)] == L
    tok = mbpe.Tokenizer(O.GPT4_SPLIT_PATTERN)
    tok.train_from_iterator(TEXTS, VOCAB, conflict_resolution=cr, device_split=split, repeats=FINE)
    assert [tuple(x) for x in tok.merges().tolist()] == ref.merges
    assert _model(tok, tmp_path) == O.model_bytes(O.GPT4_SPLIT_PATTERN, ref.merges)
    before = _snapshot(tok, tmp_path)
    # a shared pair reaches 2^31: refused, and the tokenizer is what it was
    with pytest.raises(mbpe.MbpeError) as e:
        tok.train_from_iterator(TEXTS, VOCAB + 5, conflict_resolution=cr, device_split=split, repeats=TOO_MANY)
    assert e.value.code == mbpe.ERR_OVERFLOW
    assert _snapshot(tok, tmp_path) == before
    # the session was closed: the next one opens and trains
    tok.train_from_iterator(TEXTS[::-1], 256 + 5, conflict_resolution=cr, device_split=split, repeats=FINE[::-1])
    assert len(tok.merges()) == 5 and tok.merges().tolist()[0] == [97, 98]


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("first_mode", MODES)
def test_resume_at_the_limit(tmp_path, first_mode, split):
    cr = 0 if first_mode else 1
    tok = mbpe.Tokenizer(O.GPT4_SPLIT_PATTERN)
    tok.train_from_iterator(TEXTS, 256 + 3, conflict_resolution=cr, device_split=split, repeats=[1, 1, 3])
    prior = [tuple(x) for x in tok.merges().tolist()]
    assert len(prior) == 3 and (97, 98) not in prior           # the shared pair is still there after the replay
    before = _snapshot(tok, tmp_path)
    with pytest.raises(mbpe.MbpeError) as e:
        tok.train_from_iterator(TEXTS, VOCAB, conflict_resolution=cr, device_split=split, resume=True, repeats=TOO_MANY)
    assert e.value.code == mbpe.ERR_OVERFLOW
    assert _snapshot(tok, tmp_path) == before
    _, ref = _reference(FINE, first_mode, prior=prior)
    tok.train_from_iterator(TEXTS, VOCAB, conflict_resolution=cr, device_split=split, resume=True, repeats=FINE)
    assert [tuple(x) for x in tok.merges().tolist()] == prior + ref.merges
    assert _model(tok, tmp_path) == O.model_bytes(O.GPT4_SPLIT_PATTERN, prior + ref.merges)


def _cli(*args):
    return subprocess.run([CLI] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


def test_cli_input_list_prints_the_counts_and_refuses_the_overflow(tmp_path):
    # the command line is the one place that shows the counts of a training in pieces
    paths = []
    for k, t in enumerate(TEXTS):
        paths.append(tmp_path / ("text%d.txt" % k))
        paths[-1].write_bytes(t)
    _, ref = _reference(FINE, True)
    lst, model = tmp_path / "list.txt", tmp_path / "out.model"
    lst.write_text("".join("%s\t%d\n" % (p, rep) for p, rep in zip(paths, FINE)))
    r = _cli("--train", "--input-list", lst, "-m", model, "--vocab-size", VOCAB, "-c", "first", "-v")
    assert r.returncode == 0, r.stdout + r.stderr
    shown = re.findall(r"^merge \d+/\d+: \((\d+), (\d+)\) -> \d+ .* had (-?\d+) occurrences$", r.stdout, re.M)
    assert [(int(a), int(b)) for a, b, _ in shown] == ref.merges and [int(c) for _, _, c in shown] == ref.counts
    assert model.read_bytes() == O.model_bytes(O.GPT4_SPLIT_PATTERN, ref.merges)
    lst.write_text("".join("%s\t%d\n" % (p, rep) for p, rep in zip(paths, TOO_MANY)))
    refused = tmp_path / "refused.model"
    r = _cli("--train", "--input-list", lst, "-m", refused, "--vocab-size", VOCAB, "-c", "first", "-v")
    assert r.returncode != 0 and "2^31" in r.stderr
    assert not refused.exists()
