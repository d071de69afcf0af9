"""Tokenizer.count_from_iterator / count_files / train_from_counts and `minbpe-cc --count`, `--counts`: the counting stage
run by several tokenizers or processes, each on a share of the pieces, and one training on the merged counts.
taylorswift.txt cut into 5 pieces, pieces [0:2] counted by one Tokenizer and [2:5] by another, must give, byte for byte,
the golden model of the whole text -- on every split route and across routes, merged as a tree, in two stages with
resume=True, with further texts after a blob, and through the command line, whose output must be that of
`--train --input-list` over all five files."""
import ctypes
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


@pytest.fixture(scope="module")
def gpt4_counts(pieces):
    """Pieces [0:2] and [2:5] counted by two tokenizers on the host-split route: computed once, never changed."""
    return (mbpe.Tokenizer(O.GPT4_SPLIT_PATTERN).count_from_iterator(pieces[:2]),
            mbpe.Tokenizer(O.GPT4_SPLIT_PATTERN).count_from_iterator(pieces[2:]))


def _saved(tok, tmp_path):
    path = str(tmp_path / "out.model")
    tok.save(path)
    with open(path, "rb") as f:
        return f.read()


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("name,enc,cr", CHUNKED, ids=[g[0] for g in CHUNKED])
def test_two_tables_give_the_golden_model(tmp_path, pieces, name, enc, cr, split):
    a = mbpe.Tokenizer(PATTERN[enc]).count_from_iterator(pieces[:2], device_split=split)
    b = mbpe.Tokenizer(PATTERN[enc]).count_from_iterator(iter(pieces[2:]), device_split=split)
    tok = mbpe.Tokenizer(PATTERN[enc])
    assert len(tok.merges()) == 0
    tok.train_from_counts([a, b], 512, conflict_resolution=cr)
    assert _saved(tok, tmp_path) == read_golden(name + ".model")


def test_tables_counted_on_different_split_routes(tmp_path, pieces, gpt4_counts):
    b = mbpe.Tokenizer(O.GPT4_SPLIT_PATTERN).count_from_iterator(pieces[2:], device_split=True)
    assert b == gpt4_counts[1]                       # the same chunks, so the same bytes
    tok = mbpe.Tokenizer(O.GPT4_SPLIT_PATTERN)
    tok.train_from_counts([gpt4_counts[0], b], 512, conflict_resolution=0, device_split=True)
    assert _saved(tok, tmp_path) == read_golden("taylorswift_gpt4_first_512.model")


def test_three_tables_merged_as_a_tree(tmp_path, pieces, gpt4_counts):
    counter = mbpe.Tokenizer(O.GPT4_SPLIT_PATTERN)
    a = gpt4_counts[0]
    b = counter.count_from_iterator(pieces[2:3])
    c = counter.count_from_iterator(pieces[3:])
    bc = counter.count_from_iterator([], counts=[b, c])
    assert bc == gpt4_counts[1]
    # a checkpointed count: a's table, then the rest of the pieces
    assert counter.count_from_iterator(pieces[2:], counts=[a]) == counter.count_from_iterator(pieces) == \
        counter.count_from_iterator([], counts=[a, bc])
    assert len(counter.merges()) == 0                # counting trains nothing
    tok = mbpe.Tokenizer(O.GPT4_SPLIT_PATTERN)
    tok.train_from_counts([a, bc], 512, conflict_resolution=0)
    assert _saved(tok, tmp_path) == read_golden("taylorswift_gpt4_first_512.model")


def test_resume_in_two_stages(tmp_path, gpt4_counts):
    tok = mbpe.Tokenizer(O.GPT4_SPLIT_PATTERN)
    tok.train_from_counts(gpt4_counts, 300)
    assert len(tok.merges()) == 44
    tok.train_from_counts(gpt4_counts, 512, resume=True)
    assert _saved(tok, tmp_path) == read_golden("taylorswift_gpt4_lexical_512.model")
    with pytest.raises(mbpe.MbpeError) as e:
        tok.train_from_counts(gpt4_counts, 400, resume=True)
    assert e.value.code == mbpe.ERR_ARG
    assert len(tok.merges()) == 256


@pytest.mark.parametrize("split", [False, True], ids=["host-split", "device-split"])
def test_texts_after_a_blob(tmp_path, pieces, split):
    blob = mbpe.Tokenizer(O.GPT4_SPLIT_PATTERN).count_from_iterator(pieces[:4])
    tok = mbpe.Tokenizer(O.GPT4_SPLIT_PATTERN)
    tok.train_from_counts([blob], 512, conflict_resolution=0, texts=[pieces[4]], device_split=split)
    assert _saved(tok, tmp_path) == read_golden("taylorswift_gpt4_first_512.model")


def test_count_files_reads_one_file_at_a_time(tmp_path, pieces, gpt4_counts):
    paths = []
    for k, p in enumerate(pieces[:2]):
        paths.append(str(tmp_path / ("piece%d.txt" % k)))
        with open(paths[-1], "wb") as f:
            f.write(p)
    assert mbpe.Tokenizer(O.GPT4_SPLIT_PATTERN).count_files(paths, device_split=True) == gpt4_counts[0]


def test_a_blob_of_another_pattern_is_refused(pieces, gpt4_counts):
    other = mbpe.Tokenizer(O.GPT2_SPLIT_PATTERN).count_from_iterator(pieces[2:])
    tok = mbpe.Tokenizer(O.GPT4_SPLIT_PATTERN)
    tok.train_from_counts([gpt4_counts[0]], 270)
    before = tok.merges().tolist()
    assert len(before) == 14
    for blobs in ([gpt4_counts[0], other], [gpt4_counts[0][:-16]], [gpt4_counts[0][:20]], [b"x" * 200]):
        with pytest.raises(mbpe.MbpeError) as e:
            tok.train_from_counts(blobs, 300)
        assert e.value.code == mbpe.ERR_ARG
        assert tok.merges().tolist() == before
        with pytest.raises(mbpe.MbpeError) as e:
            tok.count_from_iterator([], counts=blobs)
        assert e.value.code == mbpe.ERR_ARG
    # the session was closed: the next one opens
    tok.train_from_counts([gpt4_counts[0]], 260)
    assert len(tok.merges()) == 4


def test_the_c_calls_and_the_session(gpt4_counts):
    L = mbpe.lib()
    tok = mbpe.Tokenizer(O.GPT4_SPLIT_PATTERN)
    n = ctypes.c_uint64()
    blob = np.frombuffer(gpt4_counts[0], dtype=np.uint8)
    out = np.zeros(len(blob), dtype=np.uint8)
    # without a session
    assert L.mbpe_tok_train_pieces_export_size(tok._h, ctypes.byref(n)) == mbpe.ERR_STATE
    assert L.mbpe_tok_train_pieces_export(tok._h, out.ctypes.data, len(out), ctypes.byref(n)) == mbpe.ERR_STATE
    assert L.mbpe_tok_train_pieces_merge(tok._h, blob.ctypes.data, len(blob)) == mbpe.ERR_STATE
    # with one: a merge into the empty session is an import, and the export is the blob again; the session goes on
    assert L.mbpe_tok_train_pieces_begin(tok._h, 0, 0) == mbpe.OK
    assert L.mbpe_tok_train_pieces_merge(tok._h, blob.ctypes.data, len(blob)) == mbpe.OK
    assert L.mbpe_tok_train_pieces_export_size(tok._h, ctypes.byref(n)) == mbpe.OK and n.value == len(blob)
    assert L.mbpe_tok_train_pieces_export(tok._h, out.ctypes.data, len(out) - 1, ctypes.byref(n)) == mbpe.ERR_ARG
    assert L.mbpe_tok_train_pieces_export(tok._h, out.ctypes.data, len(out), ctypes.byref(n)) == mbpe.OK
    assert out.tobytes() == gpt4_counts[0]
    assert L.mbpe_tok_train_pieces_merge(tok._h, blob.ctypes.data, len(blob) - 16) == mbpe.ERR_ARG
    assert L.mbpe_tok_train_pieces_export(tok._h, out.ctypes.data, len(out), None) == mbpe.OK
    assert out.tobytes() == gpt4_counts[0]           # a refused merge leaves the session as it was
    assert L.mbpe_tok_train_pieces_abort(tok._h) == mbpe.OK
    assert L.mbpe_tok_train_pieces_export_size(tok._h, ctypes.byref(n)) == mbpe.ERR_STATE
    assert len(tok.merges()) == 0


def _cli(*args):
    return subprocess.run([CLI] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


def _lines(stdout):
    return [x for x in stdout.splitlines() if x.startswith(("merge ", "Split input", "Length of training"))]


@pytest.fixture(scope="module")
def lists(tmp_path_factory, pieces):
    """-> (list of all five files, list of the first two, list of the last three, the files)."""
    d = tmp_path_factory.mktemp("count-pieces")
    paths = []
    for k, p in enumerate(pieces):
        paths.append(d / ("piece%d.txt" % k))
        paths[-1].write_bytes(p)
    out = []
    for name, part in (("all.txt", paths), ("head.txt", paths[:2]), ("tail.txt", paths[2:])):
        out.append(d / name)
        out[-1].write_text("".join("%s\n" % p for p in part))
    return out + [paths]


@pytest.mark.parametrize("flags", [["-c", "lexical"], ["-c", "first", "--device-split"]],
                         ids=["lexical-host-split", "first-device-split"])
def test_cli_count_twice_then_train_on_the_counts(tmp_path, lists, gpt4_counts, flags):
    all_list, head, tail, _ = lists
    split = flags[2:]
    whole, reduced = tmp_path / "whole.model", tmp_path / "reduced.model"
    a, b = tmp_path / "a.wc", tmp_path / "b.wc"
    r = _cli("--train", "--input-list", all_list, "-m", whole, "--vocab-size", 400, "-v", "-w", *flags)
    assert r.returncode == 0, r.stdout + r.stderr
    want = _lines(r.stdout)
    assert len(want) == 144 + 2
    for lst, out in ((head, a), (tail, b)):
        r = _cli("--count", "--input-list", lst, "--counts-out", out, "-m", tmp_path / "never.model", *split)
        assert r.returncode == 0, r.stdout + r.stderr
    assert (a.read_bytes(), b.read_bytes()) == gpt4_counts
    assert not (tmp_path / "never.model").exists()    # counting writes no model
    r = _cli("--train", "--counts", a, "--counts", b, "-m", reduced, "--vocab-size", 400, "-v", "-w", *flags)
    assert r.returncode == 0, r.stdout + r.stderr
    assert _lines(r.stdout) == want
    assert reduced.read_bytes() == whole.read_bytes()
    assert (tmp_path / "reduced.model.vocab").read_bytes() == (tmp_path / "whole.model.vocab").read_bytes()
    # a counting run continued from a checkpoint, and the two tables merged without any piece: the same bytes
    ckpt, merged = tmp_path / "ckpt.wc", tmp_path / "merged.wc"
    r = _cli("--count", "--counts", a, "--input-list", tail, "--counts-out", ckpt, *split)
    assert r.returncode == 0, r.stdout + r.stderr
    r = _cli("--count", "--counts", a, "--counts", b, "--counts-out", merged)
    assert r.returncode == 0, r.stdout + r.stderr
    assert ckpt.read_bytes() == merged.read_bytes()
    assert merged.read_bytes() == mbpe.Tokenizer(O.GPT4_SPLIT_PATTERN).count_from_iterator([], counts=gpt4_counts)


def test_cli_counts_before_the_pieces_of_an_input_list(tmp_path, lists, gpt4_counts):
    _, _, tail, _ = lists
    a, model = tmp_path / "a.wc", tmp_path / "m.model"
    a.write_bytes(gpt4_counts[0])
    r = _cli("--train", "--counts", a, "--input-list", tail, "-m", model, "-c", "lexical")
    assert r.returncode == 0, r.stdout + r.stderr
    assert model.read_bytes() == read_golden("taylorswift_gpt4_lexical_512.model")


def test_cli_argument_errors(tmp_path, lists, gpt4_counts):
    all_list, head, _, paths = lists
    model, out = tmp_path / "m.model", tmp_path / "out.wc"
    a = tmp_path / "a.wc"
    a.write_bytes(gpt4_counts[0])
    r = _cli("--train", "--counts", a, "-i", paths[0], "-m", model)
    assert r.returncode != 0 and "--counts excludes --input" in r.stderr
    r = _cli("--encode", "--counts", a, "-i", paths[0], "-m", model, "-o", tmp_path / "x")
    assert r.returncode != 0 and "--counts requires --train or --count" in r.stderr
    r = _cli("--count", "--input-list", head)
    assert r.returncode != 0 and "--count requires --counts-out" in r.stderr
    r = _cli("--train", "--input-list", head, "--counts-out", out, "-m", model)
    assert r.returncode != 0 and "--counts-out requires --count" in r.stderr
    r = _cli("--count", "--train", "--input-list", head, "--counts-out", out)
    assert r.returncode != 0 and "--count excludes" in r.stderr
    r = _cli("--count", "-i", paths[0], "--counts-out", out)
    assert r.returncode != 0 and "--input-list" in r.stderr
    r = _cli("--count", "--counts-out", out)
    assert r.returncode != 0 and "Input file not specified" in r.stderr
    r = _cli("--train", "--counts")
    assert r.returncode == 106
    r = _cli("--train", "--counts", tmp_path / "missing.wc", "-m", model)
    assert r.returncode != 0 and "missing.wc does not exist" in r.stderr
    bad = tmp_path / "bad.wc"
    for content in (gpt4_counts[0][:-16], gpt4_counts[0][:10], b""):
        bad.write_bytes(content)
        r = _cli("--train", "--counts", a, "--counts", bad, "-m", model)
        assert r.returncode != 0 and "bad.wc was refused" in r.stderr
        r = _cli("--count", "--counts", bad, "--input-list", head, "--counts-out", out)
        assert r.returncode != 0 and "bad.wc was refused" in r.stderr
    # counted under another encoder
    r = _cli("--train", "--counts", a, "--encoder", "gpt2", "-m", model)
    assert r.returncode != 0 and "another split pattern" in r.stderr
    assert not model.exists() and not out.exists()
