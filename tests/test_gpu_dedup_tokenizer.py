"""Tokenizer.train(dedup=True) and `minbpe-cc --train --dedup`: split, deduplicate the chunks on the device, train on
the distinct ones with their counts.  The saved model must be, byte for byte, the golden file of the plain training --
for both tie-breaks, on every split route, in two stages with resume=True, and for a tokenizer without a pattern, whose
one chunk passes through."""
import os
import subprocess

import pytest

import mbpe
import oracle as O
from conftest import GOLDEN, ROOT, read_data, read_golden

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "minbpe-cc_amd", "minbpe-cc")
SAMPLE = os.path.join(GOLDEN, "data", "sample.txt")
PATTERN = {"gpt4": O.GPT4_SPLIT_PATTERN, "gpt2": O.GPT2_SPLIT_PATTERN, "basic": ""}
SPLITS = [pytest.param(False, id="host-split"), pytest.param(True, id="device-split"),
          pytest.param("unicode", id="device-split-unicode")]
# (fixture, text, encoder, conflict_resolution)
CHUNKED = [("taylorswift_gpt4_lexical_512", "taylorswift.txt", "gpt4", 1),
           ("taylorswift_gpt4_first_512", "taylorswift.txt", "gpt4", 0),
           ("taylorswift_gpt2_lexical_512", "taylorswift.txt", "gpt2", 1),
           ("shakespeare_gpt4_lexical_512", "shakespeare.txt", "gpt4", 1)]
BASIC = [("taylorswift_basic_lexical_512", "taylorswift.txt", "basic", 1),
         ("taylorswift_basic_first_512", "taylorswift.txt", "basic", 0)]


def _saved(tok, tmp_path):
    path = str(tmp_path / "out.model")
    tok.save(path)
    with open(path, "rb") as f:
        return f.read()


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("name,text,enc,cr", CHUNKED, ids=[g[0] for g in CHUNKED])
def test_dedup_gives_the_golden_model(tmp_path, name, text, enc, cr, split):
    tok = mbpe.Tokenizer(PATTERN[enc])
    tok.train(read_data(text), 512, conflict_resolution=cr, device_split=split, dedup=True)
    assert _saved(tok, tmp_path) == read_golden(name + ".model")


@pytest.mark.parametrize("name,text,enc,cr", BASIC, ids=[g[0] for g in BASIC])
def test_dedup_without_a_pattern_passes_through(tmp_path, name, text, enc, cr):
    tok = mbpe.Tokenizer(PATTERN[enc])
    tok.train(read_data(text), 512, conflict_resolution=cr, dedup=True)
    assert _saved(tok, tmp_path) == read_golden(name + ".model")


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("cr", [1, 0], ids=["lexical", "first"])
def test_dedup_with_resume_in_two_stages(tmp_path, cr, split):
    data = read_data("taylorswift.txt")
    half = str(tmp_path / "half.model")
    a = mbpe.Tokenizer(O.GPT4_SPLIT_PATTERN)
    a.train(data, 384, conflict_resolution=cr, device_split=split, dedup=True)
    a.save(half)
    b = mbpe.Tokenizer("")
    b.load(half)
    assert len(b.merges()) == 128
    b.train(data, 512, conflict_resolution=cr, device_split=split, resume=True, dedup=True)
    assert _saved(b, tmp_path) == read_golden("taylorswift_gpt4_%s_512.model" % ("lexical" if cr else "first"))
    # the switch is per call: the same tokenizer trains the plain way again
    b.train(data, 300, conflict_resolution=cr)
    assert len(b.merges()) == 44


def _cli(*args):
    return subprocess.run([CLI] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("cr", ["lexical", "first"])
def test_cli_dedup_writes_the_same_model(tmp_path, cr):
    plain, dedup, split = tmp_path / "plain.model", tmp_path / "dedup.model", tmp_path / "split.model"
    r = _cli("--train", "-i", SAMPLE, "-m", plain, "-c", cr, "--vocab-size", 400, "-v")
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [x for x in r.stdout.splitlines() if x.startswith(("merge ", "Split input", "Length of training"))]
    r = _cli("--train", "--dedup", "-i", SAMPLE, "-m", dedup, "-c", cr, "--vocab-size", 400, "-v")
    assert r.returncode == 0, r.stdout + r.stderr
    assert dedup.read_bytes() == plain.read_bytes()
    # the verbose lines too: counts and the final length are those of the whole corpus
    assert [x for x in r.stdout.splitlines() if x.startswith(("merge ", "Split input", "Length of training"))] == lines
    assert len(lines) == 144 + 2
    r = _cli("--train", "--dedup", "--device-split", "-i", SAMPLE, "-m", split, "-c", cr, "--vocab-size", 400)
    assert r.returncode == 0, r.stdout + r.stderr
    assert split.read_bytes() == plain.read_bytes()
