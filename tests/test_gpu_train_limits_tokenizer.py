"""The stopping rules through the tokenizer: Tokenizer.train(min_frequency=, max_token_length=), train_from_iterator and
`minbpe-cc --train --min-frequency --max-token-length`, on taylorswift.txt with the gpt4 pattern, vocab 512, at most 4
bytes per token and at least 3 occurrences, for both tie-breaks.  The reference is train_limits_cases.limited_bpe on
the host split's chunks, deduplicated in Python; every route must give its merges."""
import functools
import os
import re
import subprocess

import pytest

import mbpe
import oracle as O
import dedup_cases as C
import train_limits_cases as T
from conftest import DATA, ROOT, read_data

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "minbpe-cc_amd", "minbpe-cc")
TEXT = "taylorswift.txt"
L, F, VOCAB = 4, 3, 512
CRS = [pytest.param(1, id="lexical"), pytest.param(0, id="first")]


@functools.lru_cache(maxsize=None)
def _chunks():
    data = read_data(TEXT)
    return C.dedup(C.chunks_of(data, mbpe.presplit(O.GPT4_SPLIT_PATTERN, data)))[:2]


@functools.lru_cache(maxsize=None)
def _want(cr):
    uniq, weights = _chunks()
    m, c, _ = T.limited_bpe(uniq, weights, VOCAB, cr == 0, L=L, f=F, trace=False)
    return [list(p) for p in m]


def _saved(tok, tmp_path, name="out.model"):
    path = str(tmp_path / name)
    tok.save(path)
    with open(path, "rb") as f:
        return f.read()


@pytest.mark.parametrize("cr", CRS)
def test_every_route_gives_the_reference(tmp_path, cr):
    data = read_data(TEXT)
    want = _want(cr)
    assert want and max(T.token_lengths(want)) <= L
    tok = mbpe.Tokenizer(O.GPT4_SPLIT_PATTERN)
    tok.train(data, VOCAB, conflict_resolution=cr, dedup=True, min_frequency=F, max_token_length=L)
    assert tok.merges().tolist() == want
    model = _saved(tok, tmp_path)
    # the limits changed the result: the plain training makes longer tokens
    tok.train(data, VOCAB, conflict_resolution=cr, dedup=True)
    assert max(T.token_lengths(tok.merges())) > L
    for kw in ({}, {"device_split": True, "dedup": True}):          # the host split without dedup; the device split
        tok.train(data, VOCAB, conflict_resolution=cr, min_frequency=F, max_token_length=L, **kw)
        assert tok.merges().tolist() == want, kw
        assert _saved(tok, tmp_path) == model
    # four pieces, cut where a letter is followed by whitespace
    cuts = [0]
    for q in (1, 2, 3):
        cuts.append(re.compile(rb"[A-Za-z](?=\s)").search(data, len(data) * q // 4).end())
    pieces = [data[a:b] for a, b in zip(cuts, cuts[1:] + [len(data)])]
    tok.train_from_iterator(pieces, VOCAB, conflict_resolution=cr, min_frequency=F, max_token_length=L)
    assert tok.merges().tolist() == want
    # the command line writes the same model
    out = tmp_path / "cli.model"
    r = subprocess.run([CLI, "--train", "--dedup", "--max-token-length", str(L), "--min-frequency", str(F), "-i",
                        os.path.join(DATA, TEXT), "-m", str(out), "-c", "lexical" if cr else "first", "--vocab-size",
                        str(VOCAB), "--encoder", "gpt4"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert out.read_bytes() == model


@pytest.mark.parametrize("cr", CRS)
def test_resume_continues_a_limit_free_model(cr):
    data = read_data(TEXT)
    uniq, weights = _chunks()
    tok = mbpe.Tokenizer(O.GPT4_SPLIT_PATTERN)
    tok.train(data, 256 + 300, conflict_resolution=cr, dedup=True)
    prior = [tuple(p) for p in tok.merges().tolist()]
    assert len(prior) == 300 and max(T.token_lengths(prior)) > L
    m, _, _ = T.limited_bpe(uniq, weights, 256 + 340, cr == 0, L=L, f=F, start=(T.apply_merges(uniq, prior), 300, prior),
                            trace=False)
    assert m
    tok.train(data, 256 + 340, conflict_resolution=cr, dedup=True, resume=True, min_frequency=F, max_token_length=L)
    got = [tuple(p) for p in tok.merges().tolist()]
    assert got == prior + m
    assert max(T.token_lengths(got)[256 + 300:]) <= L


def test_the_flags_need_train(tmp_path):
    r = subprocess.run([CLI, "--encode", "--max-token-length", "4", "-i", os.path.join(DATA, TEXT), "-o",
                        str(tmp_path / "x.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--train" in r.stderr
    tok = mbpe.Tokenizer(O.GPT4_SPLIT_PATTERN)
    with pytest.raises(mbpe.MbpeError) as e:
        tok.train(b"abc abc", 260, max_token_length=1)
    assert e.value.code == mbpe.ERR_ARG
