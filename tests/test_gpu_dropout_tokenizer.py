"""BPE-dropout at the Tokenizer level on the GPU: the host loop, the device over the host split and the device split
against each other and against the oracle of tests/dropout_cases.py, in the coordinates of the buffer each route
hands the encoder; a batch of documents; the command line's --dropout / --seed on all three routes."""
import os
import subprocess

import numpy as np
import pytest

import mbpe
import oracle as O
import dropout_cases as D
from byteoff_cases import parse_special
from conftest import DATA, ROOT, read_data, read_golden
from test_encode_rank_cpu import _special_chunks

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "minbpe-cc_amd", "minbpe-cc")
P, SEED = 0.1, 3
TH = D.threshold_of(P)


def tokenizer(model, specials=False):
    pattern, _, merges = O.parse_model(read_golden(model + ".model"))
    t = mbpe.Tokenizer(pattern)
    if specials:
        t.set_special_tokens_from_file(read_data("special1.txt"))
    t.set_merges(merges)
    return t, pattern, merges


def device_split_reference(pattern, text, specials, merges, seed, threshold):
    """the device split reads the original text: every occurrence of a special token is a single, the rest is split by
    the pattern -> the oracle's tokens in the text's own coordinates"""
    off, singles, pos = [0], [], 0
    while pos < len(text):
        hits = [(text.find(n, pos), n) for n in specials if text.find(n, pos) >= 0]
        at, name = min(hits) if hits else (len(text), None)
        if at > pos:
            off += (pos + mbpe.presplit(pattern, np.frombuffer(text[pos:at], dtype=np.uint8))[1:]).tolist()
        if name is None:
            break
        singles.append((at, len(name), specials[name]))
        off.append(at + len(name))
        pos = at + len(name)
    return D.reference(text, np.array(off, dtype=np.uint64), merges, seed, threshold, singles=singles)[0]


def test_three_routes_agree_on_plain_text():
    t, pattern, merges = tokenizer("shakespeare_gpt4_lexical_512")
    text = read_data("shakespeare.txt")[:65536]
    off = mbpe.presplit(pattern, np.frombuffer(text, dtype=np.uint8))
    want = D.reference(text, off, merges, SEED, TH)[0]
    host = t.encode(text, order="rank", dropout=P, seed=SEED)
    assert np.array_equal(host, want)
    for split in (False, True, "unicode"):
        got = t.encode(text, device=0, device_split=split, order="rank", dropout=P, seed=SEED)
        assert np.array_equal(got, want), split
        got, ranges = t.encode(text, device=0, device_split=split, order="rank", dropout=P, seed=SEED, byte_ranges=True)
        assert np.array_equal(got, want), split
        assert np.array_equal(ranges, t.encode(text, order="rank", dropout=P, seed=SEED, byte_ranges=True)[1]), split
    # p = 0 through the same kept encoder is plain rank order again, and greedy with p > 0 is refused on the device too
    assert np.array_equal(t.encode(text, device=0, order="rank"), t.encode(text, order="rank"))
    for split in (False, True):
        with pytest.raises(mbpe.MbpeError) as e:
            t.encode(text, device=0, device_split=split, order="greedy", dropout=P)
        assert e.value.code == mbpe.ERR_ARG
    assert np.array_equal(t.encode(text, device=0), t.encode(text))
    t.close()


def test_special_tokens_follow_the_buffer_of_their_route():
    t, pattern, merges = tokenizer("taylorswift_gpt4_first_512", specials=True)
    specials = parse_special(read_data("special1.txt"))
    text = read_data("specialtokensample.txt")
    buf, off = _special_chunks(pattern, text, specials)                 # matches and "\0<id>" markers
    want = D.reference(buf, off, merges, SEED, TH)[0]
    assert set(specials.values()) & set(want.tolist())
    host = t.encode(text, order="rank", dropout=P, seed=SEED)
    assert np.array_equal(host, want)
    assert np.array_equal(t.encode(text, device=0, order="rank", dropout=P, seed=SEED), want)
    want_split = device_split_reference(pattern, text, specials, merges, SEED, TH)
    got = t.encode(text, device=0, device_split=True, order="rank", dropout=P, seed=SEED)
    assert np.array_equal(got, want_split)
    assert t.decode(got) == t.decode(host) == text


@pytest.mark.parametrize("split", [False, True], ids=["host-split", "device-split"])
def test_batch_of_documents(split):
    t, pattern, merges = tokenizer("shakespeare_gpt4_lexical_512")
    sh = read_data("shakespeare.txt")
    docs = [sh[:3000], b"", sh[3000:3100], sh[50000:57001], b"x"]
    joined = b"".join(docs)
    off, start = [0], 0
    for d in docs:                                                      # every document is split on its own
        if d:
            off += (start + mbpe.presplit(pattern, np.frombuffer(d, dtype=np.uint8))[1:]).tolist()
        start += len(d)
    tok, end, _, _ = D.reference(joined, np.array(off, dtype=np.uint64), merges, SEED, TH)
    doc_byte = np.concatenate([[0], np.cumsum([len(d) for d in docs])])
    chunk_tok = np.concatenate([[0], np.flatnonzero(end) + 1])
    doc_tok = chunk_tok[np.searchsorted(np.array(off), doc_byte)]
    want = [tok[a:b] for a, b in zip(doc_tok[:-1], doc_tok[1:])]
    assert len(want[1]) == 0 and all(len(w) for k, w in enumerate(want) if k != 1)
    got = t.encode_batch(docs, device_split=split, order="rank", dropout=P, seed=SEED)
    assert [g.tolist() for g in got] == [w.tolist() for w in want]
    # positions run over the joined buffer: a document on its own draws differently unless it is the first
    alone = t.encode(docs[3], device=0, device_split=split, order="rank", dropout=P, seed=SEED)
    assert not np.array_equal(alone, want[3])
    assert np.array_equal(t.encode(docs[0], device=0, device_split=split, order="rank", dropout=P, seed=SEED), want[0])
    kw = dict(seq_len=64, layout="packed", pad_id=0, eos_id=50000)
    want_ids, want_len = mbpe.pack_tokens(tok, doc_tok, **kw)
    ids, lengths = t.encode_batch_padded(docs, device_split=split, order="rank", dropout=P, seed=SEED, **kw)
    assert np.array_equal(ids, want_ids) and np.array_equal(lengths, want_len)
    aux = t.encode_batch_aux(docs, device_split=split, order="rank", dropout=P, seed=SEED, labels=True, **kw)
    assert np.array_equal(aux["ids"], want_ids)
    assert np.array_equal(aux["labels"], mbpe.pack_tokens_aux(tok, doc_tok, labels=True, **kw)["labels"])
    t.close()


def test_cli_dropout_on_all_three_routes(tmp_path):
    t, _, _ = tokenizer("taylorswift_gpt4_first_512", specials=True)
    model = tmp_path / "m.model"
    t.save(model)
    src = os.path.join(DATA, "specialtokensample.txt")
    text = read_data("specialtokensample.txt")
    base = [CLI, "--encode", "--input", src, "--model-path", str(model)]
    routes = (([], dict()), (["--device-encode"], dict(device=0)),
              (["--device-encode", "--device-split"], dict(device=0, device_split=True)))
    for k, (flags, kw) in enumerate(routes):
        out, rng = tmp_path / ("enc%d" % k), tmp_path / ("ranges%d" % k)
        r = subprocess.run(base + ["--output", str(out), "--rank-order", "--dropout", "0.1", "--seed", "3",
                                   "--byte-ranges-out", str(rng)] + flags, capture_output=True, text=True)
        assert r.returncode == 0 and "Success" in r.stdout, r.stdout + r.stderr
        want_t, want_r = t.encode(text, order="rank", dropout=0.1, seed=3, byte_ranges=True, **kw)
        assert np.frombuffer(out.read_bytes(), dtype="<u4").tolist() == want_t.tolist(), flags
        assert [[int(v) for v in ln.split()] for ln in rng.read_text().splitlines()] == want_r.tolist(), flags
        plain = tmp_path / ("plain%d" % k)
        r = subprocess.run(base + ["--output", str(plain), "--rank-order", "--dropout=0.1", "--seed=3"] + flags,
                           capture_output=True, text=True)
        assert r.returncode == 0 and plain.read_bytes() == out.read_bytes(), r.stdout + r.stderr
    # usage errors: without --rank-order, and a probability outside [0, 1]
    out = tmp_path / "never"
    r = subprocess.run(base + ["--output", str(out), "--dropout", "0.1"], capture_output=True, text=True)
    assert r.returncode != 0 and "--rank-order" in r.stderr and not out.exists()
    r = subprocess.run(base + ["--output", str(out), "--rank-order", "--dropout", "1.5"], capture_output=True, text=True)
    assert r.returncode != 0 and not out.exists()
    t.close()
