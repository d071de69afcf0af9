"""Continuing a training beyond the 16-bit slot format through the Tokenizer binding (train(..., resume=True)) and the
command line (--train --continue-from): on a corpus whose merges still have counts of 6 and more past id 65,535, train
to 65,000 (mixed case: the handover at id 65,518 lies ahead) and to 65,700 (direct case: the model already holds
17-bit ids), save, load into a fresh tokenizer, continue to 66,000 -- the bytes of the saved model must be those of
the uninterrupted training, which tests/test_gpu_cli.py::test_e2e_gpt4_vocab_100000 pins to the oracle.

A `first` training of this corpus takes 3.7 s on an MI355X, against 1.2 s in lexical mode, and the plain form of this
test makes four of them.  So `first` keeps one: the Trainer run that also shows the counts; the models to continue
from are written from its first merges, and the continuation itself goes through Tokenizer.load / train(resume=True)
as in lexical mode."""
import os
import subprocess
import time

import numpy as np
import pytest

import mbpe
import oracle as O
from conftest import ROOT

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "minbpe-cc_amd", "minbpe-cc")
VOCAB = 66000
MODES = {"lexical": 1, "first": 0}
N_WORDS = 7000


def _corpus():
    """7,000 random words of 24 lowercase letters, 6-14 occurrences each, shuffled, single spaces between them: the gpt4
    split gives one chunk per word.  (4,200 such words run out of pairs that occur near 47,400 merges -- 26 letters
    share their bigrams across words -- so the count of words is what carries real counts past id 65,535.)"""
    rng = np.random.default_rng(81)
    words = rng.integers(97, 123, size=(N_WORDS, 24), dtype=np.uint8)
    occ = np.repeat(np.arange(N_WORDS), rng.integers(6, 15, size=N_WORDS))
    rng.shuffle(occ)
    text = np.full((len(occ), 25), 32, dtype=np.uint8)
    text[:, :24] = words[occ]
    return text.reshape(-1)[:-1].tobytes()


_cache = {}


def _reference(name):
    """(corpus, model bytes of the uninterrupted Tokenizer.train to 66,000), once per tie-break; the Trainer run on the
    same chunks shows that no compared merge has a count below 2"""
    if "data" not in _cache:
        _cache["data"] = _corpus()
    data = _cache["data"]
    if name not in _cache:
        t0 = time.time()
        off = mbpe.presplit(O.GPT4_SPLIT_PATTERN, data)
        assert len(off) - 1 == data.count(b" ") + 1
        with mbpe.Trainer(0) as tr:
            tr.set_option("first_wide", 1)
            m, c, _ = tr.train(np.frombuffer(data, dtype=np.uint8), VOCAB, off, conflict_resolution=MODES[name])
        assert len(m) == VOCAB - 256 and int(m.max()) > 65535 and int(c.min()) >= 2, (len(m), int(c.min()))
        t1 = time.time()
        if name == "lexical":
            tok = mbpe.Tokenizer(O.GPT4_SPLIT_PATTERN)
            tok.train(data, VOCAB, conflict_resolution=MODES[name])
            assert tok.merges().tolist() == m.tolist()
        # (`first`: 3.7 s per training of this corpus, so the Trainer run on the tokenizer's own chunks stands for it)
        print(name, "reference: Trainer.train %.2f s, Tokenizer.train %.2f s, lowest count %d"
              % (t1 - t0, time.time() - t1, int(c.min())))
        _cache[name] = (m, O.model_bytes(O.GPT4_SPLIT_PATTERN, m))
    return (data,) + _cache[name]


@pytest.mark.parametrize("stop", [65000, 65700], ids=["mixed-from-65000", "direct-from-65700"])
@pytest.mark.parametrize("name", ["lexical", "first"])
def test_resume_gives_the_uninterrupted_model(tmp_path, name, stop):
    data, ref_m, want = _reference(name)
    part, full = str(tmp_path / "part.model"), str(tmp_path / "full.model")
    t0 = time.time()
    if name == "lexical":
        a = mbpe.Tokenizer(O.GPT4_SPLIT_PATTERN)
        a.train(data, stop, conflict_resolution=MODES[name])
        a.save(part)
    else:
        # `first`: the model a training to `stop` saves is the reference's first merges (tests/test_gpu_resume.py and
        # the lexical case above hold that); written directly, it spares 3.7 s per case
        with open(part, "wb") as f:
            f.write(O.model_bytes(O.GPT4_SPLIT_PATTERN, ref_m[:stop - 256]))
    t1 = time.time()
    b = mbpe.Tokenizer("")                      # (the pattern comes with the model)
    b.load(part)
    assert len(b.merges()) == stop - 256
    b.train(data, VOCAB, conflict_resolution=MODES[name], resume=True)
    print(name, stop, "train %.2f s, resume %.2f s" % (t1 - t0, time.time() - t1))
    assert len(b.merges()) == VOCAB - 256
    b.save(full)
    with open(full, "rb") as f:
        assert f.read() == want


def _cli(*args):
    return subprocess.run([CLI] + [str(a) for a in args], capture_output=True, text=True, timeout=300)


def test_cli_continue_from_direct(tmp_path):
    data, _, want = _reference("lexical")
    src, part, full = tmp_path / "corpus.txt", tmp_path / "part.model", tmp_path / "full.model"
    enc, dec = tmp_path / "enc", tmp_path / "dec"
    src.write_bytes(data)
    r = _cli("--train", "-i", src, "-m", part, "-c", "lexical", "--vocab-size", 65700)
    assert r.returncode == 0, r.stdout + r.stderr
    r = _cli("--train", "--continue-from", part, "-i", src, "-m", full, "-c", "lexical", "--vocab-size", VOCAB)
    assert r.returncode == 0, r.stdout + r.stderr
    assert full.read_bytes() == want
    r = _cli("--encode", "--device-encode", "--rank-order", "-i", src, "-m", full, "-o", enc)
    assert r.returncode == 0, r.stdout + r.stderr
    assert int(np.fromfile(str(enc), dtype=np.uint32).max()) > 65535
    r = _cli("--decode", "-i", enc, "-m", full, "-o", dec)
    assert r.returncode == 0, r.stdout + r.stderr
    assert dec.read_bytes() == data
