"""Tokenizer.train_from_iterator / train_files and `minbpe-cc --train --input-list`: a corpus in pieces, its chunks counted
on the device, trained on the counts.  taylorswift.txt cut into 5 pieces where a letter or digit is followed by
whitespace must give, byte for byte, the golden model of the whole text -- on every split route, in two stages with
resume=True, and through the command line, whose output must be that of `--input taylorswift.txt --dedup`."""
import os
import subprocess

import numpy as np
import pytest

import mbpe
import oracle as O
import dedup_cases as C
import wordcount_cases as W
from conftest import GOLDEN, ROOT, read_data, read_golden

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "minbpe-cc_amd", "minbpe-cc")
TAYLOR = os.path.join(GOLDEN, "data", "taylorswift.txt")
PATTERN = {"gpt4": O.GPT4_SPLIT_PATTERN, "gpt2": O.GPT2_SPLIT_PATTERN}
SPLITS = [pytest.param(False, id="host-split"), pytest.param(True, id="device-split"),
          pytest.param("unicode", id="device-split-unicode")]
# (fixture, encoder, conflict_resolution)
CHUNKED = [("taylorswift_gpt4_lexical_512", "gpt4", 1), ("taylorswift_gpt4_first_512", "gpt4", 0),
           ("taylorswift_gpt2_lexical_512", "gpt2", 1)]


@pytest.fixture(scope="module")
def pieces():
    data = read_data("taylorswift.txt")
    out = W.cut_text(data, 5)
    # the precondition: under both patterns the pieces' chunk lists laid end to end are the whole text's
    for pattern in PATTERN.values():
        assert W.concat([C.chunks_of(p, mbpe.presplit(pattern, p)) for p in out]) == \
            C.chunks_of(data, mbpe.presplit(pattern, data))
    return out


def _saved(tok, tmp_path):
    path = str(tmp_path / "out.model")
    tok.save(path)
    with open(path, "rb") as f:
        return f.read()


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("name,enc,cr", CHUNKED, ids=[g[0] for g in CHUNKED])
def test_pieces_give_the_golden_model(tmp_path, pieces, name, enc, cr, split):
    tok = mbpe.Tokenizer(PATTERN[enc])
    tok.train_from_iterator(iter(pieces), 512, conflict_resolution=cr, device_split=split)
    assert _saved(tok, tmp_path) == read_golden(name + ".model")


def test_train_files_reads_one_file_at_a_time(tmp_path, pieces):
    paths = []
    for k, p in enumerate(pieces):
        paths.append(str(tmp_path / ("piece%d.txt" % k)))
        with open(paths[-1], "wb") as f:
            f.write(p)
    tok = mbpe.Tokenizer(O.GPT4_SPLIT_PATTERN)
    tok.train_files(paths, 512, conflict_resolution=1, device_split=True)
    assert _saved(tok, tmp_path) == read_golden("taylorswift_gpt4_lexical_512.model")


@pytest.mark.parametrize("mode", [O.LEXICAL, O.FIRST], ids=["lexical", "first"])
def test_without_a_pattern_a_piece_is_one_chunk(mode):
    data = read_data("small.txt")
    parts = W.cut_list(data, 3)
    off = np.cumsum([0] + [len(p) for p in parts]).astype(np.uint64)
    want_m, _ = O.train(np.frombuffer(data, dtype=np.uint8), 256 + 30, off, mode)
    tok = mbpe.Tokenizer("")
    tok.train_from_iterator(parts, 256 + 30, conflict_resolution=1 if mode == O.LEXICAL else 0)
    assert tok.merges().tolist() == want_m.tolist()


@pytest.mark.parametrize("split", SPLITS)
def test_resume_in_two_stages(tmp_path, pieces, split):
    tok = mbpe.Tokenizer(O.GPT4_SPLIT_PATTERN)
    tok.train_from_iterator(pieces, 300, device_split=split)
    assert len(tok.merges()) == 44
    tok.train_from_iterator(pieces, 512, device_split=split, resume=True)
    assert _saved(tok, tmp_path) == read_golden("taylorswift_gpt4_lexical_512.model")
    # below the tokens the model has: refused, and nothing changes
    with pytest.raises(mbpe.MbpeError) as e:
        tok.train_from_iterator(pieces, 400, resume=True)
    assert e.value.code == mbpe.ERR_ARG
    assert len(tok.merges()) == 256
    # the session was closed: the next one opens
    tok.train_from_iterator(pieces[:1], 260)
    assert len(tok.merges()) == 4


def test_repeats_count_a_piece_several_times(pieces):
    a = mbpe.Tokenizer(O.GPT4_SPLIT_PATTERN)
    a.train_from_iterator(pieces[:3], 300, conflict_resolution=0, repeats=[1, 3, 2])
    b = mbpe.Tokenizer(O.GPT4_SPLIT_PATTERN)
    b.train_from_iterator([pieces[0]] + [pieces[1]] * 3 + [pieces[2]] * 2, 300, conflict_resolution=0)
    assert a.merges().tolist() == b.merges().tolist()
    c = mbpe.Tokenizer(O.GPT4_SPLIT_PATTERN)
    c.train_from_iterator(pieces[:3], 300, conflict_resolution=0)
    assert c.merges().tolist() != a.merges().tolist()


def test_a_failed_add_leaves_the_merges(pieces):
    tok = mbpe.Tokenizer(r"[a-z]+|[^a-z]+")            # a custom pattern has no device split
    tok.train_from_iterator(pieces[:1], 270)
    before = tok.merges().tolist()
    assert len(before) == 14
    with pytest.raises(mbpe.MbpeError) as e:
        tok.train_from_iterator(pieces, 300, device_split=True)
    assert e.value.code == mbpe.ERR_ARG
    assert tok.merges().tolist() == before

    def broken():
        yield pieces[0]
        raise KeyError("the iterator fails")

    with pytest.raises(KeyError):
        tok.train_from_iterator(broken(), 300)
    assert tok.merges().tolist() == before
    # the same at the C-ABI: the add is what fails, the session stays open until it is aborted
    L = mbpe.lib()
    text = np.frombuffer(pieces[0], dtype=np.uint8)
    assert L.mbpe_tok_train_pieces_begin(tok._h, 0, 1) == mbpe.OK
    assert L.mbpe_tok_train_pieces_add(tok._h, text.ctypes.data, len(text), 1) == mbpe.ERR_ARG
    assert L.mbpe_tok_train_pieces_begin(tok._h, 0, 1) == mbpe.ERR_STATE
    assert L.mbpe_tok_train_pieces_abort(tok._h) == mbpe.OK
    assert tok.merges().tolist() == before
    # the calls out of order
    assert L.mbpe_tok_train_pieces_begin(tok._h, 0, 0) == mbpe.OK
    assert L.mbpe_tok_train_pieces_begin(tok._h, 0, 0) == mbpe.ERR_STATE
    assert L.mbpe_tok_train_pieces_add(tok._h, None, 0, 0) == mbpe.ERR_ARG
    assert L.mbpe_tok_train_pieces_abort(tok._h) == mbpe.OK
    assert L.mbpe_tok_train_pieces_finish(tok._h, 300, 1, 0, 0) == mbpe.ERR_STATE
    assert tok.merges().tolist() == before


def _cli(*args):
    return subprocess.run([CLI] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


def _lines(stdout):
    return [x for x in stdout.splitlines() if x.startswith(("merge ", "Split input", "Length of training", "Starting"))]


@pytest.fixture(scope="module")
def piece_list(tmp_path_factory, pieces):
    d = tmp_path_factory.mktemp("pieces")
    lines = []
    for k, p in enumerate(pieces):
        path = d / ("piece%d.txt" % k)
        path.write_bytes(p)
        lines.append(str(path) + ("\t1" if k == 2 else ""))
    lst = d / "list.txt"
    lst.write_text("\n".join(lines[:2]) + "\n\n" + "\n".join(lines[2:]) + "\n")
    return lst


@pytest.mark.parametrize("flags", [["-c", "lexical"], ["-c", "first", "--device-split"],
                                   ["-c", "lexical", "--device-split-unicode"]],
                         ids=["lexical-host-split", "first-device-split", "lexical-device-split-unicode"])
def test_cli_input_list_equals_the_whole_file_with_dedup(tmp_path, piece_list, flags):
    whole, listed = tmp_path / "whole.model", tmp_path / "listed.model"
    r = _cli("--train", "--dedup", "-i", TAYLOR, "-m", whole, "--vocab-size", 400, "-v", "-w", *flags)
    assert r.returncode == 0, r.stdout + r.stderr
    want = _lines(r.stdout)
    assert len(want) == 144 + 3
    r = _cli("--train", "--input-list", piece_list, "-m", listed, "--vocab-size", 400, "-v", "-w", *flags)
    assert r.returncode == 0, r.stdout + r.stderr
    assert _lines(r.stdout) == want
    assert r.stdout.count("Loading file ") == 5
    assert listed.read_bytes() == whole.read_bytes()
    assert (tmp_path / "listed.model.vocab").read_bytes() == (tmp_path / "whole.model.vocab").read_bytes()


def test_cli_input_list_continues_a_model(tmp_path, piece_list):
    half, full = tmp_path / "half.model", tmp_path / "full.model"
    r = _cli("--train", "--input-list", piece_list, "-m", half, "--vocab-size", 300, "-c", "lexical")
    assert r.returncode == 0, r.stdout + r.stderr
    r = _cli("--train", "--input-list", piece_list, "--continue-from", half, "-m", full, "--vocab-size", 512, "-c", "lexical")
    assert r.returncode == 0, r.stdout + r.stderr
    assert full.read_bytes() == read_golden("taylorswift_gpt4_lexical_512.model")


def test_cli_input_list_repeat_and_argument_errors(tmp_path, piece_list, pieces):
    model = tmp_path / "m.model"
    r = _cli("--train", "--input-list", piece_list, "-i", TAYLOR, "-m", model)
    assert r.returncode != 0 and "--input-list excludes --input" in r.stderr
    r = _cli("--encode", "--input-list", piece_list, "-m", model, "-o", tmp_path / "x")
    assert r.returncode != 0 and "--input-list requires --train" in r.stderr
    r = _cli("--train", "--input-list", tmp_path / "missing.txt", "-m", model)
    assert r.returncode != 0 and "does not exist" in r.stderr
    r = _cli("--train", "--input-list")
    assert r.returncode == 106
    for bad in ("0", "x", "-2", "3x"):
        lst = tmp_path / "bad.txt"
        lst.write_text("%s\t%s\n" % (TAYLOR, bad))
        r = _cli("--train", "--input-list", lst, "-m", model)
        assert r.returncode == 104 and "invalid repeat count" in r.stderr, bad
    lst = tmp_path / "gone.txt"
    lst.write_text("%s\n%s\n" % (TAYLOR, tmp_path / "no-such-piece.txt"))
    r = _cli("--train", "--input-list", lst, "-m", model)
    assert r.returncode != 0 and "no-such-piece.txt does not exist" in r.stderr
    assert not model.exists()
    # a repeat count: the piece counts that many times
    files = piece_list.read_text().split()
    files = [f for f in files if f != "1"]
    lst = tmp_path / "rep.txt"
    lst.write_text("%s\n%s\t3\n" % (files[0], files[1]))
    r = _cli("--train", "--input-list", lst, "-m", model, "--vocab-size", 300)
    assert r.returncode == 0, r.stdout + r.stderr
    tok = mbpe.Tokenizer(O.GPT4_SPLIT_PATTERN)
    tok.train_from_iterator(pieces[:2], 300, conflict_resolution=0, repeats=[1, 3])
    want = tmp_path / "want.model"
    tok.save(str(want))
    assert model.read_bytes() == want.read_bytes()
