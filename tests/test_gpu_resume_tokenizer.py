"""Continuing a training through the Tokenizer binding (train(..., resume=True)) and the command line
(--train --continue-from): train to 384, save, load into a fresh tokenizer, continue to 512 -- the bytes of the saved
model must be the golden file of the uninterrupted training."""
import os
import subprocess

import pytest

import mbpe
import oracle as O
from conftest import GOLDEN, ROOT, read_data, read_golden

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "minbpe-cc_amd", "minbpe-cc")
TAYLOR = os.path.join(GOLDEN, "data", "taylorswift.txt")
GOLD = {1: "taylorswift_gpt4_lexical_512.model", 0: "taylorswift_gpt4_first_512.model"}


def _two_stages(tmp_path, cr, **kw):
    data = read_data("taylorswift.txt")
    half, full = str(tmp_path / "half.model"), str(tmp_path / "full.model")
    a = mbpe.Tokenizer(O.GPT4_SPLIT_PATTERN)
    a.train(data, 384, conflict_resolution=cr, **kw)
    a.save(half)
    b = mbpe.Tokenizer("")                      # (the pattern comes with the model)
    b.load(half)
    assert len(b.merges()) == 128
    b.train(data, 512, conflict_resolution=cr, resume=True, **kw)
    assert len(b.merges()) == 256
    b.save(full)
    with open(full, "rb") as f:
        return f.read(), b


@pytest.mark.parametrize("cr", [1, 0], ids=["lexical", "first"])
@pytest.mark.parametrize("split", [False, True, "unicode"], ids=["host-split", "device-split", "device-split-unicode"])
def test_resume_gives_the_golden_model(tmp_path, cr, split):
    blob, tok = _two_stages(tmp_path, cr, device_split=split)
    assert blob == read_golden(GOLD[cr])
    sample = read_data("sample.txt")
    assert tok.decode(tok.encode(sample)) == sample


def test_resume_without_merges_is_train():
    tok = mbpe.Tokenizer(O.GPT4_SPLIT_PATTERN)
    tok.train(read_data("taylorswift.txt"), 512, resume=True)
    assert O.model_bytes(O.GPT4_SPLIT_PATTERN, tok.merges()) == read_golden(GOLD[1])


def test_resume_keeps_special_tokens_and_refuses_a_smaller_vocab(tmp_path):
    data = read_data("taylorswift.txt")
    tok = mbpe.Tokenizer(O.GPT4_SPLIT_PATTERN)
    tok.train(data, 384)
    tok.set_special_tokens_from_file(read_data("special1.txt"))
    with pytest.raises(mbpe.MbpeError) as e:
        tok.train(data, 300, resume=True)
    assert e.value.code == mbpe.ERR_ARG
    assert len(tok.merges()) == 128                                # refused before anything was dropped
    tok.train(data, 512, resume=True)
    path = str(tmp_path / "with-specials.model")
    tok.save(path)
    with open(path, "rb") as f:
        pattern, specials, merges = O.parse_model(f.read())
    words = read_data("special1.txt").decode("utf-8").split()
    want_specials = list(zip(words[::2], [int(w) for w in words[1::2]]))
    assert pattern == O.GPT4_SPLIT_PATTERN and sorted(specials) == sorted(want_specials) and specials
    assert merges.tolist() == O.parse_model(read_golden(GOLD[1]))[2].tolist()
    src = read_data("specialtokensample.txt")
    assert tok.decode(tok.encode(src)) == src


def _cli(*args):
    return subprocess.run([CLI] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("cr", ["lexical", "first"])
def test_cli_continue_from(tmp_path, cr):
    half, full = tmp_path / "half.model", tmp_path / "full.model"
    r = _cli("--train", "-i", TAYLOR, "-m", half, "-c", cr, "--vocab-size", 384)
    assert r.returncode == 0, r.stdout + r.stderr
    r = _cli("--train", "--continue-from", half, "-i", TAYLOR, "-m", full, "-c", cr, "--vocab-size", 512, "-v",
             "--encoder", "basic")                                 # (no effect: the model's pattern is used)
    assert r.returncode == 0, r.stdout + r.stderr
    assert full.read_bytes() == read_golden(GOLD[1 if cr == "lexical" else 0])
    assert "merge 129/256:" in r.stdout and "merge 128/256:" not in r.stdout and "merge 256/256:" in r.stdout
    # a vocabulary below the loaded model's: an error exit, and no model written
    small = tmp_path / "small.model"
    r = _cli("--train", "--continue-from", full, "-i", TAYLOR, "-m", small, "-c", cr, "--vocab-size", 400)
    assert r.returncode != 0 and "400" in r.stderr, r.stdout + r.stderr
    assert not small.exists()
    r = _cli("--train", "--continue-from", tmp_path / "missing.model", "-i", TAYLOR, "-m", small)
    assert r.returncode != 0 and not small.exists()
