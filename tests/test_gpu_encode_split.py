"""Encode from a text and an end mask that are on the device already (mbpe_encoder_encode_endmask,
mbpe_encoder_encode_batch_endmask) against mbpe_encoder_encode / _batch / _batch_aux with the chunk offsets read off
the same mask; then the Tokenizer, the C-ABI switch and the command line with the device split against the host
split."""
import os
import subprocess

import numpy as np
import pytest

import mbpe
import oracle as O
import split_cases as S
from conftest import DATA, ROOT, read_data, read_golden

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "minbpe-cc_amd", "minbpe-cc")


def golden_merges(name):
    return O.parse_model(read_golden(name + ".model"))[2]


@pytest.fixture(scope="module")
def dev():
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


class Case:
    """A text with its chunk offsets on the host and, on the device, the text and the end mask of those chunks."""

    def __init__(self, dev, data, chunk_off, doc_chunk_off):
        self.data = np.ascontiguousarray(np.frombuffer(bytes(data), dtype=np.uint8))
        self.off = np.ascontiguousarray(chunk_off, dtype=np.uint64)
        assert (self.off[1:] > self.off[:-1]).all()               # a mask has no empty chunk
        self.doc_chunk = np.ascontiguousarray(doc_chunk_off, dtype=np.uint64)
        self.doc_off = self.off[self.doc_chunk.astype(np.int64)]
        n = len(self.data)
        bits = np.zeros(mbpe.Splitter.mask_bytes(n) * 8, dtype=np.uint8)
        bits[self.off[1:].astype(np.int64) - 1] = 1
        self.d_text = torch.from_numpy(self.data.copy()).to(dev)
        self.d_mask = torch.from_numpy(np.packbits(bits, bitorder="little")).to(dev)
        torch.cuda.synchronize()

    def ptrs(self):
        return self.d_text.data_ptr(), len(self.data), self.d_mask.data_ptr()


def random_documents(seed, n_chunks):
    """n_chunks chunks grouped into documents of 0 .. 3 chunks -> chunk index of every document's first chunk."""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(0, 4, n_chunks)
    cum = np.concatenate([[0], np.cumsum(sizes)])
    cum = cum[cum < n_chunks]
    return np.concatenate([cum, [n_chunks, n_chunks]]).astype(np.uint64)      # (and an empty document at the end)


@pytest.fixture(scope="module")
def shakespeare(dev):
    data = read_data("shakespeare.txt")
    off = mbpe.presplit(S.PATTERNS["gpt4"], np.frombuffer(data, dtype=np.uint8))
    return Case(dev, data, off, random_documents(5, len(off) - 1))


@pytest.fixture(scope="module")
def encoder(dev):
    with mbpe.Encoder(golden_merges("shakespeare_gpt4_lexical_512")) as enc:
        yield enc


@pytest.fixture(scope="module")
def reference(shakespeare, encoder):
    """mbpe_encoder_encode of the same chunks, once."""
    tokens, chunk_tok_off = encoder.encode(shakespeare.data, shakespeare.off, offsets=True)
    tokens.setflags(write=False)
    return tokens, chunk_tok_off


def test_tokens_and_document_offsets(shakespeare, encoder, reference):
    c = shakespeare
    want, chunk_tok_off = reference
    want_doc = chunk_tok_off[c.doc_chunk.astype(np.int64)]
    got, doc_tok = encoder.encode_endmask(*c.ptrs(), doc_off=c.doc_off)
    assert len(got) == len(want) and (got == want).all()
    assert (doc_tok == want_doc).all()
    # every chunk its own document: every rank there is, on every word and block edge of the popcount
    got, doc_tok = encoder.encode_endmask(*c.ptrs(), doc_off=c.off)
    assert (got == want).all() and (doc_tok == chunk_tok_off).all()
    # without documents; 16-bit ids
    got, doc_tok = encoder.encode_endmask(*c.ptrs())
    assert doc_tok is None and (got == want).all()
    got, doc_tok = encoder.encode_endmask(*c.ptrs(), doc_off=c.doc_off, dtype=np.uint16)
    assert got.dtype == np.uint16 and (got == want).all() and (doc_tok == want_doc).all()
    # the query, and a cap that is too small: the count, no token, no offset beyond [0]
    n, doc_tok = encoder.encode_endmask(*c.ptrs(), doc_off=c.doc_off, query=True)
    assert n == len(want) and (doc_tok == want_doc).all()
    with pytest.raises(mbpe.MbpeError) as e:
        encoder.encode_endmask(*c.ptrs(), doc_off=c.doc_off, cap=len(want) - 1)
    assert e.value.code == mbpe.ERR_ARG


@pytest.mark.parametrize("bits", [32, 16])
def test_device_output(dev, shakespeare, encoder, reference, bits):
    c = shakespeare
    want, chunk_tok_off = reference
    out = torch.zeros(len(c.data), dtype=torch.int32 if bits == 32 else torch.int16, device=dev)
    torch.cuda.synchronize()
    n, doc_tok = encoder.encode_endmask(*c.ptrs(), doc_off=c.doc_off, dtype=np.uint32 if bits == 32 else np.uint16,
                                        out_ptr=out.data_ptr(), cap=len(c.data))
    assert n == len(want) and (doc_tok == chunk_tok_off[c.doc_chunk.astype(np.int64)]).all()
    got = out.cpu().numpy()[:n].view(np.uint32 if bits == 32 else np.uint16)
    if bits == 32:                                                # bit 31 = last token of its chunk
        flags = np.flatnonzero(got >> 31)
        assert (flags == chunk_tok_off[1:].astype(np.int64) - 1).all()
        got = got & 0x7FFFFFFF
    assert (got == want).all()
    assert not out.cpu().numpy()[n:].any()
    # a cap too small writes nothing
    out.zero_()
    torch.cuda.synchronize()
    with pytest.raises(mbpe.MbpeError) as e:
        encoder.encode_endmask(*c.ptrs(), out_ptr=out.data_ptr(), cap=n - 1, dtype=np.uint32 if bits == 32 else np.uint16)
    assert e.value.code == mbpe.ERR_ARG and not out.cpu().numpy().any()


@pytest.mark.parametrize("n_bytes", [1, 31, 32, 33, 1024, 1025, 2047, 2048, 2049, 4097])
def test_one_byte_chunks_around_span_and_block_edges(dev, n_bytes):
    # no pair merges: n_bytes tokens, every byte a chunk and a document of its own -- more chunk ends than half the
    # bytes (the list of ends has a buffer of its own), ranks 0 .. n_bytes
    data = bytes((7 * k) % 26 + 97 for k in range(n_bytes))
    off = np.arange(n_bytes + 1, dtype=np.uint64)
    c = Case(dev, data, off, np.arange(n_bytes + 1))
    with mbpe.Encoder(np.array([[255, 255]], dtype=np.uint32)) as enc:
        want, chunk_tok_off = enc.encode(c.data, c.off, offsets=True)
        got, doc_tok = enc.encode_endmask(*c.ptrs(), doc_off=c.doc_off)
        assert len(got) == n_bytes and (got == want).all() and (doc_tok == chunk_tok_off).all()
        docs = np.array([0, 0, n_bytes // 2, n_bytes, n_bytes], dtype=np.uint64)
        got, doc_tok = enc.encode_endmask(*c.ptrs(), doc_off=docs)
        assert (doc_tok == docs).all()


def test_singles(dev, encoder):
    # the text holds names, the caller says which ranges are one token: those chunks become their id, all others
    # are what mbpe_encoder_encode makes of them
    text = b"First Citizen:<|e|>Before we proceed<|e|><|fim|> any further, hear me speak.<|e|>"
    names = {b"<|e|>": 100257, b"<|fim|>": 300}
    pieces, at = [], 0
    while at < len(text):
        hit = min(((text.find(k, at), k) for k in names if text.find(k, at) >= 0), default=(len(text), None))
        if hit[0] > at:
            pieces.append((at, hit[0], None))
        if hit[1] is not None:
            pieces.append((hit[0], hit[0] + len(hit[1]), names[hit[1]]))
        at = hit[0] + (len(hit[1]) if hit[1] else 0)
    off, want, singles = [0], [], []
    for a, b, sid in pieces:
        if sid is not None:
            off.append(b)
            want.append([sid])
            singles.append((a, b - a, sid))
            continue
        o = mbpe.presplit(S.PATTERNS["gpt4"], np.frombuffer(text[a:b], dtype=np.uint8))
        for x, y in zip(o[:-1].tolist(), o[1:].tolist()):
            off.append(a + y)
            want.append(encoder.encode(text[a + x:a + y]).tolist())
    c = Case(dev, text, off, np.arange(len(off)))
    got, doc_tok = encoder.encode_endmask(*c.ptrs(), singles=singles, doc_off=c.doc_off)
    assert got.tolist() == sum(want, [])
    assert doc_tok.tolist() == np.cumsum([0] + [len(w) for w in want]).tolist()
    with pytest.raises(mbpe.MbpeError) as e:                      # an id beyond 16 bits with 16-bit output
        encoder.encode_endmask(*c.ptrs(), singles=singles, dtype=np.uint16)
    assert e.value.code == mbpe.ERR_VOCAB
    for bad in ([singles[1], singles[0]], [singles[0], (singles[0][0] + 1, 2, 5)], [(len(text) - 1, 2, 5)], [(3, 0, 5)]):
        with pytest.raises(mbpe.MbpeError) as e:
            encoder.encode_endmask(*c.ptrs(), singles=bad)
        assert e.value.code == mbpe.ERR_ARG
    with pytest.raises(mbpe.MbpeError) as e:
        encoder.encode_endmask(*c.ptrs(), doc_off=[0, 9, 5])
    assert e.value.code == mbpe.ERR_ARG


@pytest.mark.parametrize("layout", ["padded", "packed"])
def test_batch_against_the_chunk_offset_calls(shakespeare, encoder, layout):
    c = shakespeare
    kw = dict(seq_len=37, layout=layout, pad_id=0, bos_id=None if layout == "packed" else 1, eos_id=2)
    want_ids, want_len = encoder.encode_batch(c.data, c.off, c.doc_chunk, **kw)
    ids, lengths = encoder.encode_batch_endmask(*c.ptrs(), None, c.doc_off, **kw)
    assert ids.shape == want_ids.shape and (ids == want_ids).all() and (lengths == want_len).all()
    aux = dict(labels=True, positions=True, segments=True, cu_seqlens=layout == "packed")
    want = encoder.encode_batch_aux(c.data, c.off, c.doc_chunk, **kw, **aux)
    want_doc = encoder.doc_tok_off.copy()
    got = encoder.encode_batch_endmask(*c.ptrs(), None, c.doc_off, **kw, **aux)
    assert sorted(got) == sorted(want)
    for k in want:
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), k
    assert (encoder.doc_tok_off == want_doc).all()
    ids16, len16 = encoder.encode_batch_endmask(*c.ptrs(), None, c.doc_off, out_bits=16, **kw)
    assert ids16.dtype == np.uint16 and (ids16 == want_ids).all() and (len16 == want_len).all()


def test_repeat_calls_allocate_nothing(shakespeare, encoder):
    c = shakespeare
    kw = dict(seq_len=64, layout="packed", eos_id=2)
    encoder.encode_endmask(*c.ptrs(), doc_off=c.doc_off)
    encoder.encode_batch_endmask(*c.ptrs(), None, c.doc_off, labels=True, positions=True, segments=True, **kw)
    before = encoder.alloc_count()
    for _ in range(2):
        encoder.encode_endmask(*c.ptrs(), doc_off=c.doc_off)
        encoder.encode_batch_endmask(*c.ptrs(), None, c.doc_off, labels=True, positions=True, segments=True, **kw)
    assert encoder.alloc_count() == before


def test_one_piece_only(dev):
    data = (b"some words and more words " * 400)[:8192]
    off = mbpe.presplit(S.PATTERNS["gpt4"], np.frombuffer(data, dtype=np.uint8))
    c = Case(dev, data, off, [0, len(off) - 1])
    with mbpe.Encoder(golden_merges("shakespeare_gpt4_lexical_512")) as enc:
        want = enc.encode(c.data, c.off)
        enc.set_option("piece_bytes", 4096)
        with pytest.raises(mbpe.MbpeError) as e:
            enc.encode_endmask(*c.ptrs())
        assert e.value.code == mbpe.ERR_OOM and "4096" in str(e.value) and "piece_bytes" in str(e.value)
        enc.set_option("piece_bytes", 8192)
        assert (enc.encode_endmask(*c.ptrs())[0] == want).all()


# ---- Tokenizer, C-ABI switch, command line -----------------------------------------------------------------------

@pytest.fixture(scope="module")
def tok(dev):
    t = mbpe.Tokenizer(O.GPT4_SPLIT_PATTERN)
    t.set_special_tokens_from_file(read_data("special1.txt"))
    t.set_merges(golden_merges("taylorswift_gpt4_lexical_512"))
    return t


NUL_TEXT = b"hi<|endoftext|>\x0042 x<|fim_prefix|>\x00abc  <|endoftext|><|endoftext|>  \x00 7<|endofprompt|>tail  "


@pytest.mark.parametrize("name", ["specialtokensample.txt", "taylorswift.txt", None])
def test_tokenizer_encode(tok, name):
    text = NUL_TEXT if name is None else read_data(name)
    want = tok.encode(text)                                       # the host loop
    assert tok.encode(text, device=0, device_split=True).tolist() == want.tolist()
    assert tok.encode(text, device=0).tolist() == want.tolist()   # (the switch is per call)
    assert tok.encode(b"", device=0, device_split=True).tolist() == []


def batch_texts():
    sample = read_data("specialtokensample.txt")
    swift = read_data("taylorswift.txt")
    return [sample, b"", swift[:5000], NUL_TEXT, b"a  ", b"b", b"<|endoftext|>", swift[5000:9000] + b"<|endoftext|>", b""]


def test_tokenizer_batch_calls(tok):
    texts = batch_texts()
    want = tok.encode_batch(texts, device_split=False)
    got = tok.encode_batch(texts, device_split=True)
    assert [g.tolist() for g in got] == [w.tolist() for w in want]
    assert [w.tolist() for w in want] == [tok.encode(t).tolist() for t in texts]
    for layout in ("padded", "packed"):
        kw = dict(seq_len=48, layout=layout, pad_id=0, eos_id=100257)
        a = tok.encode_batch_padded(texts, device_split=False, **kw)
        b = tok.encode_batch_padded(texts, device_split=True, **kw)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        aux = dict(labels=True, positions=True, segments=True, cu_seqlens=layout == "packed")
        a = tok.encode_batch_aux(texts, device_split=False, **kw, **aux)
        off_a = tok.doc_tok_off.copy()
        b = tok.encode_batch_aux(texts, device_split=True, **kw, **aux)
        assert sorted(a) == sorted(b)
        for k in a:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
        assert (tok.doc_tok_off == off_a).all()


def test_basic_tokenizer_has_no_device_split(dev):
    t = mbpe.Tokenizer("")
    t.set_merges(golden_merges("shakespeare_basic_lexical_512"))
    for call in (lambda: t.encode(b"abab", device=0, device_split=True),
                 lambda: t.encode_batch([b"abab", b"cd"], device_split=True),
                 lambda: t.encode_batch_padded([b"abab"], 8, device_split=True),
                 lambda: t.encode_batch_aux([b"abab"], 8, labels=True, device_split=True)):
        with pytest.raises(mbpe.MbpeError) as e:
            call()
        assert e.value.code == mbpe.ERR_ARG
    assert t.encode(b"abab", device=0).tolist() == t.encode(b"abab").tolist()     # no fallback, and no harm done


def test_cli_encode_with_the_device_split(tok, tmp_path):
    # the scenario of tests/test_gpu_cli.py: specialtokensample.txt with a gpt4 model that holds special tokens
    model = tmp_path / "m.model"
    tok.save(model)
    src = os.path.join(DATA, "specialtokensample.txt")
    outs = []
    for k, flags in enumerate(([], ["--device-encode", "--device-split"], ["--device-split"])):
        out = tmp_path / ("enc%d" % k)
        r = subprocess.run([CLI, "--encode", "--input", src, "--model-path", str(model), "--output", str(out)] + flags,
                           capture_output=True, text=True)
        assert r.returncode == 0 and "Success" in r.stdout, r.stdout + r.stderr
        outs.append(out.read_bytes())
    assert outs[0] == outs[1] == outs[2] and len(outs[0]) > 0
    assert np.frombuffer(outs[0], dtype=np.uint32).tolist() == tok.encode(read_data("specialtokensample.txt")).tolist()
