"""GPU tests of decode on the device (csrc/decode.hip: mbpe_decoder_create / mbpe_decode_tokens / mbpe_decode_slots /
mbpe_decode_stream, Tokenizer.decode(device=), --device-decode).  Expected values come from the host decode
(Tokenizer::decode, the reference's loop Tokenizer.h:725-751), from the fixtures and from the corpora themselves,
never from the device path."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import mbpe
import oracle as O
from mbpe import check
from conftest import GOLDEN, ROOT, read_data, read_golden
from test_tokenizer_cpu import SPECIAL_SAMPLE_TOKENS, _golden_merges

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "minbpe-cc_amd", "minbpe-cc")
DATA = os.path.join(GOLDEN, "data")


@pytest.fixture(scope="module")
def dev():
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def _host_tok(merges, specials=b""):
    tok = mbpe.Tokenizer("")
    if specials:
        tok.set_special_tokens_from_file(specials)
    tok.set_merges(merges)
    return tok


def _doubling(k):
    """(97,97), (256,256), ...: token 255 + j is 2^j bytes of `a`."""
    return np.array([[97, 97]] + [[255 + j, 255 + j] for j in range(1, k)], dtype=np.uint32)


# ---- 1. the encode vectors ------------------------------------------------------------------------------------------

def test_sample_with_shakespeare_basic_model():
    merges = _golden_merges("shakespeare_basic_lexical_512")
    data = read_data("sample.txt")
    tok = _host_tok(merges)
    enc = tok.encode(data)
    assert len(enc) == 15677
    with mbpe.Decoder(merges) as d:
        got, bad = d.decode(enc, with_invalid=True)
    assert got == data and bad == 0
    assert tok.decode(enc, device=0) == data == tok.decode(enc)


def test_taylorswift_with_gpt4_model():
    tok = mbpe.Tokenizer(O.GPT4_SPLIT_PATTERN)
    tok.set_merges(_golden_merges("taylorswift_gpt4_lexical_512"))
    data = read_data("taylorswift.txt")
    enc = tok.encode(data)
    assert len(enc) == 94201
    assert tok.decode(enc, device=0) == data == tok.decode(enc)


def test_special_token_sample():
    tok = mbpe.Tokenizer(O.GPT4_SPLIT_PATTERN)
    tok.set_special_tokens_from_file(read_data("special1.txt"))
    tok.set_merges(_golden_merges("taylorswift_gpt4_first_512"))
    data = read_data("specialtokensample.txt")
    assert tok.decode(SPECIAL_SAMPLE_TOKENS, device=0) == data == tok.decode(SPECIAL_SAMPLE_TOKENS)


# ---- 2. edges -------------------------------------------------------------------------------------------------------

def test_no_tokens_and_one_token():
    m = np.array([[97, 98], [256, 99]], dtype=np.uint32)
    with mbpe.Decoder(m) as d:
        assert d.decode([], with_invalid=True) == (b"", 0)
        assert d.decode([257]) == b"abc"
        assert d.decode([0]) == b"\0"
        assert d.decode([258], with_invalid=True) == (b"", 1)
    assert _host_tok(m).decode([], device=0) == b""
    with mbpe.Decoder(np.zeros((0, 2), dtype=np.uint32)) as d:
        assert d.decode([104, 105]) == b"hi"


def test_invalid_ids_are_skipped_counted_and_warned(capfd):
    m = np.array([[97, 98], [256, 99]], dtype=np.uint32)
    tokens = [257, 258, 97, 0xFFFFFFFF, 70000, 256, 0x80000000 | 97]
    with mbpe.Decoder(m) as d:
        assert d.decode(tokens, with_invalid=True) == (b"abcaab", 4)
    tok = _host_tok(m)
    capfd.readouterr()
    want = tok.decode(tokens)
    host_err = capfd.readouterr().err
    got = tok.decode(tokens, device=0)
    dev_err = capfd.readouterr().err
    assert got == want == b"abcaab"
    lines = ["Warning: Attempted to decode invalid token ID: %d" % t for t in (258, 0xFFFFFFFF, 70000, 0x80000000 | 97)]
    assert dev_err.splitlines() == host_err.splitlines() == lines * 2      # (the binding calls twice: length, bytes)


def test_specials_override_extend_and_may_be_empty():
    m = np.array([[97, 98], [256, 99]], dtype=np.uint32)
    specials = b"<|over|> 256\n<|byte|> 120\n<|far|> 70000\n<|far2|> 4294967295\n<|top|> 258\n"
    tok = _host_tok(m, specials)
    tokens = [257, 256, 120, 121, 70000, 258, 259, 0xFFFFFFFF, 97]
    want = tok.decode(tokens)
    assert want == b"abc<|over|><|byte|>y<|far|><|top|><|far2|>a"
    assert tok.decode(tokens, device=0) == want
    # vocab[257] was built from vocab[256] before the special took id 256 over: it stays "abc"
    sp = {256: b"<|over|>", 300: b"", 301: b"x", 5: b""}
    with mbpe.Decoder(m, sp) as d:
        assert d.decode([5, 256, 300, 257, 301, 302, 300], with_invalid=True) == (b"<|over|>abcx", 1)
    # of two specials with one id the later holds (special_tokens_reverse_lookup[id] = name)
    h = ctypes.c_void_p()
    ids = np.array([300, 300], dtype=np.uint32)
    blob = np.frombuffer(b"onetwo", dtype=np.uint8)
    off = np.array([0, 3, 6], dtype=np.uint64)
    assert mbpe.lib().mbpe_decoder_create(0, m.ctypes.data, 2, ids.ctypes.data, blob.ctypes.data, off.ctypes.data, 2,
                                          ctypes.byref(h)) == 0
    t = np.array([300, 97], dtype=np.uint32)
    out = np.zeros(8, dtype=np.uint8)
    n = ctypes.c_uint64()
    assert mbpe.lib().mbpe_decode_tokens(h, t.ctypes.data, 2, 0, out.ctypes.data, 8, 0, ctypes.byref(n), None) == 0
    mbpe.lib().mbpe_decoder_destroy(h)
    assert out[:n.value].tobytes() == b"twoa"


def test_merge_that_names_an_undefined_id_equals_the_host():
    # merge 1 names 300 (not yet defined) and itself; merge 2 uses the half-empty entry
    m = np.array([[97, 98], [300, 99], [257, 257], [258, 256], [260, 100]], dtype=np.uint32)
    tok = _host_tok(m)
    tokens = [256, 257, 258, 259, 260, 100]
    want = tok.decode(tokens)
    assert want == b"abcccccabdd"
    with mbpe.Decoder(m) as d:
        assert d.decode(tokens, with_invalid=True) == (want, 0)


def test_size_query_and_cap_one_too_small():
    m = _golden_merges("shakespeare_basic_lexical_512")
    tok = _host_tok(m)
    t = np.ascontiguousarray(tok.encode(read_data("small.txt")), dtype=np.uint32)
    want = tok.decode(t)
    n, bad = ctypes.c_uint64(), ctypes.c_uint64()
    with mbpe.Decoder(m) as d:
        L = mbpe.lib()
        assert L.mbpe_decode_tokens(d._h, t.ctypes.data, len(t), 0, None, 0, 0, ctypes.byref(n), ctypes.byref(bad)) == 0
        assert n.value == len(want) and bad.value == 0
        out = np.full(len(want) + 8, 0xAB, dtype=np.uint8)
        n.value = 0
        rc = L.mbpe_decode_tokens(d._h, t.ctypes.data, len(t), 0, out.ctypes.data, len(want) - 1, 0, ctypes.byref(n), None)
        assert rc == mbpe.ERR_ARG and n.value == len(want) and bool((out == 0xAB).all())
        assert L.mbpe_decode_tokens(d._h, t.ctypes.data, len(t), 0, out.ctypes.data, len(want), 0, ctypes.byref(n), None) == 0
        assert out[:len(want)].tobytes() == want and bool((out[len(want):] == 0xAB).all())


# ---- 3. shapes against the host decode ------------------------------------------------------------------------------

def test_token_counts_around_the_spans():
    m = _golden_merges("shakespeare_basic_lexical_512")
    tok = _host_tok(m)
    rng = np.random.default_rng(11)
    counts = [1023, 1024, 1025, 4095, 4096, 4097] + [int(x) for x in rng.integers(1, 1 << 22, size=3)] + [1 << 22]
    with mbpe.Decoder(m) as d:
        for n in counts:
            t = rng.integers(0, 512, size=n, dtype=np.uint32)
            assert d.decode(t) == tok.decode(t), n


def test_every_output_alignment_and_both_edge_pieces(dev):
    # a leading token of every length 0 .. 31, host and device-resident (the device buffer itself is shifted too)
    m = np.array([[97, 98], [256, 99], [257, 257], [258, 100], [259, 259], [260, 257], [261, 261]], dtype=np.uint32)
    sp = {1000 + k: bytes(range(65, 65 + k)) for k in range(32)}
    tok = _host_tok(m)                                  # (the body holds no special: the host decodes it)
    rng = np.random.default_rng(5)
    with mbpe.Decoder(m, sp) as d:
        for lead in range(32):
            body = rng.integers(0, 256 + len(m), size=int(rng.integers(1, 3000)), dtype=np.uint32)
            t = np.concatenate([[1000 + lead], body]).astype(np.uint32)
            want = bytes(range(65, 65 + lead)) + tok.decode(body)
            assert d.decode(t) == want, lead
            td = torch.from_numpy(t.astype(np.int64)).to(dev).to(torch.int32)
            buf = torch.full((len(want) + 64,), 0xEE, dtype=torch.uint8, device=dev)
            shift = lead % 16 + 1
            n, bad = d.decode_device(td.data_ptr(), len(t), buf.data_ptr() + shift, len(want))
            assert (n, bad) == (len(want), 0)
            got = buf.cpu().numpy()
            assert got[shift:shift + n].tobytes() == want, lead
            assert bool((got[:shift] == 0xEE).all()) and bool((got[shift + n:] == 0xEE).all()), lead


def test_doubling_vocabulary_with_a_64_kib_token():
    m = _doubling(16)                                   # token 271 = 65,536 bytes
    tok = _host_tok(m)
    rng = np.random.default_rng(3)
    t = rng.integers(0, 256, size=5000, dtype=np.uint32)
    t[rng.integers(0, 5000, size=40)] = 271
    t[rng.integers(0, 5000, size=200)] = rng.integers(256, 272, size=200, dtype=np.uint32)
    want = tok.decode(t)
    assert len(want) > 40 * 65536 // 2
    with mbpe.Decoder(m) as d:
        assert d.decode(t) == want


def test_a_span_that_decodes_to_nothing():
    m = np.array([[97, 98]], dtype=np.uint32)
    tok = _host_tok(m)
    t = np.concatenate([np.full(700, 256), np.full(3000, 9999), np.full(5, 97), np.full(1024, 0xFFFFFFFF),
                        np.full(3, 256)]).astype(np.uint32)
    with mbpe.Decoder(m, {9999: b""}) as d:
        got, bad = d.decode(t, with_invalid=True)
    assert got == b"ab" * 700 + b"aaaaa" + b"ababab" and bad == 1024
    assert got == tok.decode(np.where(t == 9999, 0xFFFFFFF0, t))       # (the host has no empty special: an invalid id)


# ---- 4. device-resident, and encode -> decode without the tokens visiting the host ---------------------------------

def test_encode_on_device_then_decode_on_device(dev):
    sh = read_data("shakespeare.txt")
    data = sh * 8
    merges = _golden_merges("shakespeare_gpt4_lexical_512")
    off1 = mbpe.presplit(O.GPT4_SPLIT_PATTERN, sh).astype(np.uint64)
    off = np.concatenate([off1[:-1] + np.uint64(i * len(sh)) for i in range(8)] + [np.array([len(data)], dtype=np.uint64)])
    n_tok, _ = mbpe.encode_chunks_device(data, off, merges, 0, 0)
    tokens = torch.zeros(n_tok, dtype=torch.int32, device=dev)
    n2, passes = mbpe.encode_chunks_device(data, off, merges, tokens.data_ptr(), n_tok)
    assert n2 == n_tok and passes >= 2 and n_tok < len(data)
    out = torch.zeros(len(data), dtype=torch.uint8, device=dev)
    with mbpe.Decoder(merges) as d:
        n, bad = d.decode_slots_device(tokens.data_ptr(), n_tok, 32, 0x80000000, None, out.data_ptr(), len(data))
        assert (n, bad) == (len(data), 0)
        assert d.kernel_ms() > 0
    want = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to(dev)
    assert bool(torch.equal(out, want))
    # the ids are those of the host-returning call
    enc, _ = mbpe.encode_chunks(data[:len(sh)], off1, merges)
    assert np.array_equal((tokens[:len(enc)].cpu().numpy().view(np.uint32) & 0x7FFFFFFF), enc)


# ---- 5. output beyond 4 GiB -----------------------------------------------------------------------------------------

def test_output_beyond_4_gib(dev):
    # 258 = "abcd", 261 = "efgh", 262 = "abcdefgh", nine doublings: token 271 holds 4,096 bytes
    m = np.array([[97, 98], [99, 100], [256, 257], [101, 102], [103, 104], [259, 260], [258, 261]] +
                 [[262 + j, 262 + j] for j in range(9)], dtype=np.uint32)
    big = 256 + len(m) - 1
    pat = _host_tok(m).decode([big])
    assert len(pat) == 4096 and pat[:16] == b"abcdefghabcdefgh"
    n_rep = (9 << 29) // 4096                           # 4.5 GiB
    t = torch.full((n_rep + 1,), big, dtype=torch.int32, device=dev)
    t[0] = 120                                          # one byte in front: no token starts on a 16-byte boundary
    want_len = 1 + n_rep * 4096
    assert want_len > (1 << 32)
    out = torch.empty(want_len + 15, dtype=torch.uint8, device=dev)
    out[-15:] = 0xEE
    with mbpe.Decoder(m) as d:
        assert d.decode_device(t.data_ptr(), n_rep + 1, 0, 0) == (want_len, 0)
        assert d.decode_device(t.data_ptr(), n_rep + 1, out.data_ptr(), want_len) == (want_len, 0)
    assert int(out[0]) == 120 and bool((out[-15:] == 0xEE).all())
    rows = out[1:want_len].view(n_rep, 4096)
    p = torch.from_numpy(np.frombuffer(pat, dtype=np.uint8).copy()).to(dev)
    for lo in range(0, n_rep, 1 << 16):
        assert bool((rows[lo:lo + (1 << 16)] == p).all()), lo


# ---- 6. the live stream of a training -------------------------------------------------------------------------------

def _stream_equals(tr, merges, corpus, dev):
    corpus = np.frombuffer(bytes(corpus), dtype=np.uint8)
    got = tr.decode_stream()
    assert len(got) == len(corpus)
    assert got == corpus.tobytes()
    ct = torch.from_numpy(corpus.copy()).to(dev)
    out = torch.zeros(len(corpus) + 1, dtype=torch.uint8, device=dev)
    assert tr.decode_stream_device(0, 0) == len(corpus)
    assert tr.decode_stream_device(out.data_ptr(), len(corpus)) == len(corpus)
    assert bool(torch.equal(out[:-1], ct)) and int(out[-1]) == 0
    rt = check.decode_roundtrip(tr, merges, ct, torch, dev)       # the second, independent decoder
    assert rt["ok"], rt


def test_stream_one_chunk_with_holes_and_compacted(dev):
    data = O.splitmix64_bytes(42, 16 << 20)
    with mbpe.Trainer(0) as tr:
        tr.set_option("compact_den", 0)                            # never compact: the holes stay
        tr.load_corpus(data)
        tr.train_begin(1024)
        tr.train_steps(768)
        m = tr.train_result()[0]
        assert len(m) == 768
        st = tr.stats()
        assert st["n_live"] < st["n_slots"]                        # holes are present
        assert tr.stream_device()[2:] == (16, 0, None)
        _stream_equals(tr, m, data, dev)
        tr.compact()
        _stream_equals(tr, m, data, dev)
    with mbpe.Trainer(0) as tr:                                    # mid-training, default compaction
        tr.load_corpus(data)
        tr.train_begin(1024)
        tr.train_steps(100)
        _stream_equals(tr, tr.train_result()[0], data, dev)


def test_stream_end_bit_barrier_and_wide(dev):
    data = read_data("shakespeare.txt")
    off = mbpe.presplit(O.GPT4_SPLIT_PATTERN, data)
    for option, layout in ((None, (16, 0x8000, None)), (("chunk_barrier", 1), (16, 0, 0xFFEE)),
                           (("wide_from", 100), (32, 0x80000000, None))):
        with mbpe.Trainer(0) as tr:
            if option:
                tr.set_option(*option)
            m, _, _ = tr.train_lexical(data, 512, off)
            assert len(m) == 256 and tr.stream_device()[2:] == layout
            _stream_equals(tr, m, data, dev)
    with mbpe.Trainer(0) as tr:                                    # the continuation of a one-chunk corpus
        tr.set_option("wide_from", 50)
        m, _, _ = tr.train_lexical(data, 400)
        assert tr.stream_device()[2] == 32
        _stream_equals(tr, m, data, dev)


def test_stream_of_a_corpus_given_as_ranges_with_gaps(dev):
    data = read_data("taylorswift.txt")
    starts, ends = mbpe.presplit_ranges(r"\p{L}+", data)
    packed = b"".join(data[int(s):int(e)] for s, e in zip(starts, ends))
    assert len(packed) < len(data)
    with mbpe.Trainer(0) as tr:
        tr.load_corpus_ranges(data, starts, ends)
        tr.train_begin(400)
        tr.train_steps(144)
        _stream_equals(tr, tr.train_result()[0], packed, dev)


def test_stream_before_begin_is_a_state_error():
    with mbpe.Trainer(0) as tr:
        tr.load_corpus(b"hello hello")
        with pytest.raises(mbpe.MbpeError) as e:
            tr.decode_stream()
        assert e.value.code == mbpe.ERR_STATE


# ---- 7. the command line --------------------------------------------------------------------------------------------

def test_cli_device_decode(tmp_path):
    model, enc, dec, dec2 = tmp_path / "m", tmp_path / "enc", tmp_path / "dec", tmp_path / "dec2"
    model.write_bytes(read_golden("shakespeare_basic_lexical_512.model"))
    src = os.path.join(DATA, "sample.txt")
    r = subprocess.run([CLI, "--encode", "--input", src, "--model-path", str(model), "--output", str(enc)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    outs = []
    for out, extra in ((dec, []), (dec2, ["--device-decode"])):
        r = subprocess.run([CLI, "--decode", "--input", str(enc), "--model-path", str(model), "--output", str(out)] + extra,
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        outs.append(r.stdout.replace(str(out), "OUT").split("Execution time")[0])
    assert outs[0] == outs[1]                                      # same messages
    assert dec.read_bytes() == dec2.read_bytes() == read_data("sample.txt")
