"""The device split with the option "unicode" (k_split_sync_u, k_split_walk_u in csrc/split.hip) against mbpe_presplit
on the same bytes: the texts of tests/split_unicode_cases.py through Splitter.split and Splitter.split_docs, bit for
bit and without a host span where the CPU test (test_split_unicode_cpu.py) has none; the option off on the same build;
documents and special-token names next to multi-byte characters; then Tokenizer.train, the encode calls and the command
line against the host split.  Ill-formed text is the CPU test's alone: its spans are the host's, and PCRE2, which
the library asks without a UTF check, is not defined on them."""
import os
import subprocess

import numpy as np
import pytest

import mbpe
import oracle as O
import split_cases as S
import split_docs_cases as D
import split_unicode_cases as U
from conftest import ROOT, read_data

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

ENCODERS = ["gpt2", "gpt4"]
BLOCK = mbpe.SPLIT_BLOCK
CLI = os.path.join(ROOT, "minbpe-cc_amd", "minbpe-cc")
E = b"<|endoftext|>"


@pytest.fixture(scope="module")
def dev():
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def splitters(dev):
    sp = {e: mbpe.Splitter(S.PATTERNS[e]) for e in ENCODERS}
    for s in sp.values():
        s.set_option("unicode", 1)
    yield sp
    for s in sp.values():
        s.close()


def bits_of(mask_tensor, n):
    bits = np.unpackbits(mask_tensor.cpu().numpy(), bitorder="little")
    assert not bits[n:].any(), "end bits beyond the text"
    return bits[:n].astype(bool)


def differ(encoder, blob, got, want):
    wrong = np.flatnonzero(got != want)
    assert len(wrong) == 0, "%s: %d chunk ends differ, first at byte %d: %r" % (
        encoder, len(wrong), wrong[0], bytes(blob[max(0, wrong[0] - 24):wrong[0] + 24]))


def check_text(sp, dev, encoder, data, want=None):
    """Splitter.split of one text: the device mask against end_mask_of(mbpe_presplit)."""
    data = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else data
    n = len(data)
    mask = torch.full((sp.mask_bytes(n),), 0xA5, dtype=torch.uint8, device=dev)
    n_chunks = sp.split(data, offsets=False, mask_ptr=mask.data_ptr())
    if want is None:
        want = S.end_mask_of(mbpe.presplit(S.PATTERNS[encoder], data), n)
    differ(encoder, data, bits_of(mask, n), want)
    assert n_chunks == int(want.sum())


def check_docs(sp, dev, encoder, blob, off, names=(), on_device=False, truth=None):
    """Splitter.split_docs: every document (every part of it) split as a text of its own."""
    blob = np.ascontiguousarray(blob, dtype=np.uint8)
    n = len(blob)
    want, want_ranges, _ = truth if truth is not None else D.truth(S.PATTERNS[encoder], blob, off, list(names))
    mask = torch.full((sp.mask_bytes(n),), 0xA5, dtype=torch.uint8, device=dev)
    if on_device:
        text = torch.from_numpy(blob.copy()).to(dev)
        torch.cuda.synchronize()
        n_chunks, ranges = sp.split_docs(doc_off=off, names=names, mask_ptr=mask.data_ptr(), text_ptr=text.data_ptr(),
                                         n_bytes=n)
    else:
        n_chunks, ranges = sp.split_docs(blob, off, names, mask_ptr=mask.data_ptr())
    differ(encoder, blob, bits_of(mask, n), want)
    assert n_chunks == int(want.sum())
    assert ranges.tolist() == want_ranges.tolist()


_TRUTH = {}


def truth_of(encoder, key, blob, off):
    """of documents without names (a NUL-led document is one chunk)"""
    if (encoder, key) not in _TRUTH:
        _TRUTH[(encoder, key)] = D.truth(S.PATTERNS[encoder], blob, off, [])
    return _TRUTH[(encoder, key)]


@pytest.mark.parametrize("encoder", ENCODERS)
def test_every_scalar_value_in_one_call(splitters, dev, encoder):
    blob, _ = U.every_scalar_value()
    sp = splitters[encoder]
    check_text(sp, dev, encoder, blob, S.truth_end_mask(S.PATTERNS[encoder], blob, [0, len(blob)]))
    assert sp.host_spans() == (0, 0)


@pytest.mark.parametrize("encoder", ENCODERS)
def test_pseudo_scripts(splitters, dev, encoder):
    sp = splitters[encoder]
    for name, text in sorted(U.pseudo_scripts().items()):
        try:
            check_text(sp, dev, encoder, text)
        except AssertionError as e:
            raise AssertionError("%s: %s" % (name, e))
        assert sp.host_spans() == (0, 0), name
    blob, off = D.join(U.whitespace_ends())
    check_docs(sp, dev, encoder, blob, off)
    assert sp.host_spans() == (0, 0)


@pytest.mark.parametrize("encoder", ENCODERS)
@pytest.mark.parametrize("name", ["shakespeare.txt", "taylorswift.txt", "sample.txt"])
def test_fixtures(splitters, dev, encoder, name):
    sp = splitters[encoder]
    check_text(sp, dev, encoder, read_data(name))
    assert sp.host_spans() == (0, 0)
    assert sp.kernel_ms() > 0


def test_option_off_is_the_byte_rule(dev):
    data = read_data("taylorswift.txt")
    with mbpe.Splitter(S.PATTERNS["gpt4"]) as sp:
        check_text(sp, dev, "gpt4", data)
        assert sp.host_spans() == (109, 2142)
        sp.set_option("unicode", 1)
        check_text(sp, dev, "gpt4", data)
        assert sp.host_spans() == (0, 0)
        before = sp.alloc_count()
        check_text(sp, dev, "gpt4", data)
        assert sp.alloc_count() == before               # the table is uploaded once
        sp.set_option("unicode", 0)
        check_text(sp, dev, "gpt4", data)
        assert sp.host_spans() == (109, 2142)


def test_set_option(dev):
    with mbpe.Splitter(S.PATTERNS["gpt2"]) as sp:
        for bad in (2, -1, 1 << 32):
            with pytest.raises(mbpe.MbpeError) as e:
                sp.set_option("unicode", bad)
            assert e.value.code == mbpe.ERR_ARG
        sp.set_option("unicode", 1)
        sp.set_option("unicode", 0)


@pytest.mark.parametrize("encoder", ENCODERS)
def test_alignment(splitters, dev, encoder):
    blob, off = D.join(U.alignment())
    sp = splitters[encoder]
    for on_device in (False, True):
        check_docs(sp, dev, encoder, blob, off, on_device=on_device, truth=truth_of(encoder, "alignment", blob, off))
        assert sp.host_spans() == (0, 0)


@pytest.mark.parametrize("encoder", ENCODERS)
@pytest.mark.parametrize("share", [0.08, 0.6])
def test_random_strings(splitters, dev, encoder, share):
    blob, off = S.random_strings(21, 100000, 40, S.HOSTILE, S.NON_ASCII, share)
    sp = splitters[encoder]
    check_docs(sp, dev, encoder, blob, off, truth=truth_of(encoder, "strings %g" % share, blob, off))
    assert sp.host_spans() == (0, 0)
    # the same bytes as one text: the documents' ends are no boundaries any more
    text = S.random_text(23, 1 << 20, S.HOSTILE + S.ASCII, S.NON_ASCII, share)
    check_text(sp, dev, encoder, text)
    assert sp.host_spans() == (0, 0)


@pytest.mark.parametrize("encoder", ENCODERS)
def test_every_prefix_of_three_blocks(splitters, dev, encoder):
    sp = splitters[encoder]
    text = S.random_text(32, 3 * BLOCK + 8, S.HOSTILE, S.NON_ASCII, 0.6)
    lengths = [n for n in range(0, 3 * BLOCK + 1) if (text[n] & 0xC0) != 0x80]
    blob = np.concatenate([text[:n] for n in lengths])
    check_docs(sp, dev, encoder, blob, np.cumsum([0] + lengths).astype(np.uint64))
    assert sp.host_spans() == (0, 0)
    for n in lengths[::7] + lengths[-3:]:
        check_text(sp, dev, encoder, text[:n])


@pytest.mark.parametrize("encoder", ENCODERS)
def test_spans_around_max_span(splitters, dev, encoder):
    sp = splitters[encoder]
    sp.set_option("max_span", 256)
    try:
        for body, n_host in U.max_span_texts(256):
            check_text(sp, dev, encoder, body)
            assert sp.host_spans()[0] == n_host, body[-8:]
    finally:
        sp.set_option("max_span", mbpe.SPLIT_MAX_SPAN)


def multibyte_documents():
    """Documents that begin and end with the characters of NON_ASCII, so that every cut has one on both sides; with
    <|endoftext|> between characters, and a NUL-led part."""
    chars = [c.decode() for c in S.NON_ASCII]
    docs = []
    for i, a in enumerate(chars):
        b = chars[(i + 5) % len(chars)]
        docs += [(a + "x " + b).encode(), (b + a).encode(), (a + b + " 12" + a).encode(), a.encode()]
        docs.append(a.encode() + E + b.encode() + b" t" + a.encode() + E + E + b.encode())
        docs.append(("word" + a).encode() + E + (b + "\n" + a).encode())
    docs += [b"\x00" + chars[0].encode() + b"12", chars[1].encode() * 70, E + chars[3].encode() * 33 + E]
    return docs


@pytest.mark.parametrize("encoder", ENCODERS)
@pytest.mark.parametrize("max_span", [mbpe.SPLIT_MAX_SPAN, 1])
def test_split_docs_cuts_next_to_multibyte_characters(splitters, dev, encoder, max_span):
    sp = splitters[encoder]
    blob, off = D.join(multibyte_documents())
    names = [E, "é".encode(), " t".encode()]
    sp.set_option("max_span", max_span)
    try:
        for on_device in (False, True):
            check_docs(sp, dev, encoder, blob, off, names, on_device)
            assert (sp.host_spans()[0] == 0) == (max_span > 1)
        for cid, docs, case_names in D.NAMED:                       # the default mode's cases, in this mode
            b, o = D.join(docs)
            try:
                check_docs(sp, dev, encoder, b, o, case_names)
            except AssertionError as e:
                raise AssertionError("%s: %s" % (cid, e))
    finally:
        sp.set_option("max_span", mbpe.SPLIT_MAX_SPAN)


# ---- Tokenizer, command line ----------------------------------------------------------------------------------------

def end_to_end_texts():
    return {"cyrillic": U.cyrillic(), "cjk": U.cjk(), "taylorswift": read_data("taylorswift.txt")}


@pytest.fixture(scope="module")
def trained(dev):
    """name -> (text, tokenizer trained with the host split)"""
    out = {}
    for name, text in end_to_end_texts().items():
        tok = mbpe.Tokenizer(O.GPT4_SPLIT_PATTERN)
        tok.set_special_tokens_from_file(read_data("special1.txt"))
        tok.train(text, 300, device_split=False)
        out[name] = (text, tok)
    return out


@pytest.mark.parametrize("name", ["cyrillic", "cjk", "taylorswift"])
def test_tokenizer_train(trained, name):
    text, host = trained[name]
    tok = mbpe.Tokenizer(O.GPT4_SPLIT_PATTERN)
    tok.train(text, 300, device_split="unicode")
    assert tok.merges().tolist() == host.merges().tolist()
    assert len(tok.merges()) == 300 - 256


@pytest.mark.parametrize("name", ["cyrillic", "cjk", "taylorswift"])
def test_tokenizer_encode(trained, name):
    text, tok = trained[name]
    docs = [text[:30001].decode("utf-8", "ignore").encode(), b"", text[40000:70000].decode("utf-8", "ignore").encode()]
    joined = E.join(docs)
    want = tok.encode(joined)                                     # the host loop
    assert tok.encode(joined, device=0, device_split="unicode").tolist() == want.tolist()
    assert tok.encode(joined, device=0, device_split=True).tolist() == want.tolist()      # (the switch is per call)
    texts = docs + [E, joined[:5000].decode("utf-8", "ignore").encode() + E]
    got = tok.encode_batch(texts, device_split="unicode")
    assert [g.tolist() for g in got] == [tok.encode(t).tolist() for t in texts]
    kw = dict(seq_len=48, layout="packed", pad_id=0, eos_id=100257)
    a = tok.encode_batch_padded(texts, device_split=False, **kw)
    b = tok.encode_batch_padded(texts, device_split="unicode", **kw)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    a = tok.encode_batch_aux(texts, device_split=False, labels=True, **kw)
    b = tok.encode_batch_aux(texts, device_split="unicode", labels=True, **kw)
    assert sorted(a) == sorted(b) and all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in a)


def test_cli(trained, tmp_path):
    src = tmp_path / "cjk.txt"
    src.write_bytes(U.cjk(60000) + E + U.cyrillic(20000))
    models = []
    for k, flags in enumerate(([], ["--device-split-unicode"])):
        model = tmp_path / ("m%d" % k)
        r = subprocess.run([CLI, "--train", "-i", str(src), "-m", str(model), "-c", "lexical", "--vocab-size", "300"] + flags,
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        models.append(model.read_bytes())
    assert models[0] == models[1] and len(models[0]) > 0
    model = tmp_path / "special.model"
    trained["cjk"][1].save(model)
    outs = []
    for k, flags in enumerate(([], ["--device-encode", "--device-split-unicode"])):
        out = tmp_path / ("enc%d" % k)
        r = subprocess.run([CLI, "--encode", "--input", str(src), "--model-path", str(model), "--output", str(out)] + flags,
                           capture_output=True, text=True)
        assert r.returncode == 0 and "Success" in r.stdout, r.stdout + r.stderr
        outs.append(out.read_bytes())
    assert outs[0] == outs[1] and len(outs[0]) > 0
