"""Token frequency tables on the host loop (mbpe_tok_count_tokens with device_id < 0) and the command line's
--token-counts-out: the table must be the bincount of Tokenizer.encode, text by text, with repeats; the model is a golden
one saved and loaded with special tokens whose ids (100,257 ..) lie far above 256 + n_merges."""
import os
import subprocess

import numpy as np
import pytest

import mbpe
import oracle as O
from conftest import ROOT, read_data, read_golden

CLI = os.path.join(ROOT, "minbpe-cc_amd", "minbpe-cc")
ORDERS = ("greedy", "rank")


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    tok = mbpe.Tokenizer(O.GPT4_SPLIT_PATTERN)
    tok.set_special_tokens_from_file(read_data("special1.txt"))
    tok.set_merges(O.parse_model(read_golden("taylorswift_gpt4_first_512.model"))[2])
    path = tmp_path_factory.mktemp("counts") / "sp.model"
    tok.save(path)
    return str(path)


@pytest.fixture(scope="module")
def texts():
    swift = read_data("taylorswift.txt")
    return [read_data("specialtokensample.txt"), swift[:20000], b"", b"<|endoftext|>", swift[20000:30000] + b"<|endoftext|>"]


def want_table(tok, texts, order, repeats=None):
    n_ids = 100277                                      # special1.txt: <|endofprompt|> 100276 is the largest id
    out = np.zeros(n_ids, dtype=np.uint64)
    for i, t in enumerate(texts):
        ids = tok.encode(t, order=order)
        out += np.bincount(ids, minlength=n_ids).astype(np.uint64) * np.uint64(1 if repeats is None else repeats[i])
    return out


@pytest.mark.parametrize("order", ORDERS)
def test_host_loop_is_the_bincount_of_encode(model, texts, order):
    tok = mbpe.Tokenizer("")
    tok.load(model)
    want = want_table(tok, texts, order)
    assert want[100257] == 3 and want[100258] == 1       # the special tokens are counted under their ids
    got = tok.token_counts(texts, device=None, order=order)
    assert got.dtype == np.uint64 and np.array_equal(got, want)
    # several batches, and a second call starts from zero
    assert np.array_equal(tok.token_counts(iter(texts), device=None, order=order, batch_bytes=1000), want)
    repeats = [3, 1, 7, 2, 1]
    got = tok.token_counts(texts, device=None, order=order, repeats=repeats)
    assert np.array_equal(got, want_table(tok, texts, order, repeats))
    with pytest.raises(mbpe.MbpeError) as e:
        tok.token_counts(texts, device=None, order=order, repeats=[1, 0, 1, 1, 1])
    assert e.value.code == mbpe.ERR_ARG


def test_changing_the_model_empties_the_table(model):
    tok = mbpe.Tokenizer("")
    tok.load(model)
    assert tok.token_counts([b"hello"], device=None).sum() > 0
    tok.set_special_tokens_from_file(b"<|x|> 600\n")
    assert len(tok.token_counts([], device=None)) == 601
    tok.set_merges(np.array([[104, 105]], dtype=np.uint32))
    got = tok.token_counts([b"hi<|x|>"], device=None)
    assert len(got) == 601 and got[256] == 1 and got[600] == 1 and got.sum() == 2
    # a special id at or above MBPE_MAX_COUNT_IDS
    tok.set_special_tokens_from_file(b"<|x|> 33554432\n")
    with pytest.raises(mbpe.MbpeError) as e:
        tok.token_counts([b"hi"], device=None)
    assert e.value.code == mbpe.ERR_VOCAB


def read_table(path):
    rows = [line.split() for line in open(path).read().splitlines()]
    assert [int(r[0]) for r in rows] == list(range(len(rows)))
    return np.array([int(r[1]) for r in rows], dtype=np.uint64)


@pytest.mark.parametrize("order", ORDERS)
def test_cli_token_counts_out(model, texts, order, tmp_path):
    tok = mbpe.Tokenizer("")
    tok.load(model)
    paths = []
    for i, t in enumerate(texts):
        paths.append(str(tmp_path / ("t%d.txt" % i)))
        open(paths[-1], "wb").write(t)
    flags = ["--rank-order"] if order == "rank" else []
    out = str(tmp_path / "one.counts")
    r = subprocess.run([CLI, "--encode", "--input", paths[0], "--model-path", model, "--token-counts-out", out] + flags,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert np.array_equal(read_table(out), want_table(tok, texts[:1], order))
    assert not os.path.exists(str(tmp_path / "one.counts.tokens"))
    repeats = [3, 1, 7, 2, 1]
    listing = str(tmp_path / "list.txt")
    with open(listing, "w") as f:
        for p, rep in zip(paths, repeats):
            f.write(p + ("\n" if rep == 1 else "\t%d\n" % rep))
    out = str(tmp_path / "all.counts")
    r = subprocess.run([CLI, "--encode", "--input-list", listing, "--model-path", model, "--token-counts-out", out] + flags,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert np.array_equal(read_table(out), want_table(tok, texts, order, repeats))


def test_cli_usage_errors(model, tmp_path):
    sample = str(tmp_path / "s.txt")
    open(sample, "wb").write(b"hello world")
    out = str(tmp_path / "x.counts")
    head = [CLI, "--encode", "--model-path", model, "--token-counts-out", out]
    r = subprocess.run(head + ["--input", sample, "--output", str(tmp_path / "x.tok")], capture_output=True, text=True)
    assert r.returncode == 107 and "--output" in r.stderr and not os.path.exists(out)
    r = subprocess.run([CLI, "--decode", "--input", sample, "--token-counts-out", out], capture_output=True, text=True)
    assert r.returncode == 107
    listing = str(tmp_path / "list.txt")
    open(listing, "w").write(sample + "\t0\n")
    r = subprocess.run(head + ["--input-list", listing], capture_output=True, text=True)
    assert r.returncode == 104 and "repeat" in r.stderr and not os.path.exists(out)
    # the word-count options keep their meaning
    r = subprocess.run(head + ["--input", sample, "--count"], capture_output=True, text=True)
    assert r.returncode == 107
