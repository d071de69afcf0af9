"""GPU tests of batch decode on the device (csrc/decode.hip: mbpe_decode_batch with k_dec_bounds and the plain 16-bit
ids, mbpe_tok_decode_batch_device, Decoder.decode_batch / decode_batch_device, Tokenizer.decode_batch).  Expected
values come from the host loop (Tokenizer.decode without a device, per document), from the corpora and from
arithmetic on known entry lengths, never from the device path."""
import ctypes

import numpy as np
import pytest
import torch

import mbpe
import oracle as O
from conftest import read_data
from test_tokenizer_cpu import _golden_merges

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def _host_tok(merges, specials=b"", pattern=""):
    tok = mbpe.Tokenizer(pattern)
    if specials:
        tok.set_special_tokens_from_file(specials)
    tok.set_merges(merges)
    return tok


def _doubling(k):
    """(97,97), (256,256), ...: token 255 + j is 2^j bytes of `a`."""
    return np.array([[97, 97]] + [[255 + j, 255 + j] for j in range(1, k)], dtype=np.uint32)


def _batch(d, t, off, out=None, cap=0, bits=32):
    """mbpe_decode_batch of host tokens -> (code, doc_byte_off, n, n_invalid); out: a host uint8 array or None."""
    t = np.ascontiguousarray(t, dtype=np.uint32 if bits == 32 else np.uint16)
    off = np.ascontiguousarray(off, dtype=np.uint64)
    b = np.full(len(off), 0xDEADBEEF, dtype=np.uint64)
    n, bad = ctypes.c_uint64(), ctypes.c_uint64()
    rc = mbpe.lib().mbpe_decode_batch(d._h, t.ctypes.data if len(t) else None, len(t), bits, 0, off.ctypes.data,
                                      len(off) - 1, None if out is None else out.ctypes.data, cap, 0, b.ctypes.data,
                                      ctypes.byref(n), ctypes.byref(bad))
    return rc, b, n.value, bad.value


# ---- 1. the fixtures ------------------------------------------------------------------------------------------------

def test_taylorswift_lines_round_trip():
    tok = _host_tok(_golden_merges("taylorswift_gpt4_lexical_512"), pattern=O.GPT4_SPLIT_PATTERN)
    lines = read_data("taylorswift.txt").splitlines(keepends=True)
    assert len(lines) > 900 and b"" not in lines
    enc = tok.encode_batch(lines, device=0)
    got = tok.decode_batch(enc, device=0)
    assert got == lines
    assert got == [tok.decode(e) for e in enc]
    assert tok.decode_batch([], device=0) == []
    assert tok.decode_batch([[], []], device=0) == [b"", b""]


def test_specials_and_overriding_specials_inside_documents(capfd):
    # 100257 / 100258 lie beyond the vocabulary, <|over|> takes id 300 over, 999999 decodes to nothing
    sp = read_data("special1.txt") + b"<|over|> 300\n"
    tok = _host_tok(_golden_merges("taylorswift_gpt4_first_512"), sp, O.GPT4_SPLIT_PATTERN)
    parts = [b"This is some text that contains <|fim_prefix|> two", b"", b" special <|endoftext|> tokens.",
             b"<|endoftext|>", read_data("specialtokensample.txt")]
    enc = [e.tolist() for e in tok.encode_batch(parts, device=0)]
    assert sum(e.count(100257) for e in enc) == 3 and sum(e.count(100258) for e in enc) == 2
    docs = enc + [[300, 84, 300], [999999, 104, 300, 100257, 511, 512]]
    capfd.readouterr()
    want = [tok.decode(e) for e in docs]
    host_err = capfd.readouterr().err
    assert want[:5] == parts and want[5] == b"<|over|>T<|over|>" and b"<|over|><|endoftext|>" in want[6]
    got = tok.decode_batch(docs, device=0)
    dev_err = capfd.readouterr().err
    assert got == want
    lines = ["Warning: Attempted to decode invalid token ID: %d" % t for t in (999999, 512)]
    assert dev_err.splitlines() == host_err.splitlines() == lines * 2      # (the binding calls twice: length, bytes)


# ---- 2. where a boundary falls --------------------------------------------------------------------------------------

BOUNDARIES = [0, 0, 1, 2, 500, 1023, 1024, 1024, 1025, 1500, 2047, 2048, 2049, 2999, 3000]


@pytest.mark.parametrize("n_tokens", [1, 1023, 1024, 1025, 2048, 3000])
def test_boundary_placement(n_tokens):
    m = _doubling(7)                                    # ids 256 .. 262: 2 .. 128 bytes
    tok = _host_tok(m)
    rng = np.random.default_rng(n_tokens)
    t = rng.integers(0, 256 + len(m), size=n_tokens, dtype=np.uint32)
    t[rng.integers(0, n_tokens, size=n_tokens // 9)] = 9999              # the empty special
    bad_at = np.unique(rng.integers(0, n_tokens, size=n_tokens // 11))
    t[bad_at] = 70000 + bad_at                           # invalid ids
    # (the host has no empty special: there the id is one more invalid one and decodes to nothing as well)
    lens = np.array([len(tok.decode([x])) for x in range(256 + len(m))] + [0], dtype=np.uint64)
    per_token = lens[np.minimum(t, 256 + len(m))]
    cum = np.concatenate([[0], np.cumsum(per_token, dtype=np.uint64)]).astype(np.uint64)
    off = sorted(set(b for b in BOUNDARIES if b <= n_tokens) | {0, n_tokens})
    off = [0] + off + [n_tokens]                         # (0 and n_tokens twice: an empty first and last document)
    with mbpe.Decoder(m, {9999: b""}) as d:
        flat, flat_bad = d.decode(t, with_invalid=True)
        assert flat == tok.decode(t) and len(flat) == int(cum[-1])
        assert flat_bad == len(bad_at)
        out = np.full(len(flat) + 8, 0xAB, dtype=np.uint8)
        rc, b, n, bad = _batch(d, t, off, out, len(flat))
        assert rc == 0 and n == len(flat) and bad == flat_bad
        assert b.tolist() == cum[off].tolist()
        assert out[:n].tobytes() == flat and bool((out[n:] == 0xAB).all())
        docs = [t[lo:hi] for lo, hi in zip(off[:-1], off[1:])]
        got, bad = d.decode_batch(docs, with_invalid=True)
        assert got == [tok.decode(x) for x in docs] and bad == flat_bad


# ---- 3. many boundaries in one span ---------------------------------------------------------------------------------

def test_one_token_documents_and_runs_of_empty_ones():
    m = _doubling(5)
    tok = _host_tok(m)
    rng = np.random.default_rng(8)
    t = rng.integers(0, 256 + len(m), size=1500, dtype=np.uint32)
    # 1,500 one-token documents; 200 empty ones: 70 at the very start, 40 at token 1,024 (between the last document of
    # the first span and the first of the second), 30 in the middle, 60 at the end
    empties = {0: 70, 700: 30, 1024: 40, 1500: 60}
    off = []
    for i in range(1501):
        off += [i] * (empties.get(i, 0) + 1)
    assert len(off) - 1 == 1700 and off[0] == 0 and off[-1] == 1500
    docs = [t[lo:hi] for lo, hi in zip(off[:-1], off[1:])]
    assert sum(len(x) == 0 for x in docs) == 200 and sum(len(x) == 1 for x in docs) == 1500
    want = [tok.decode(x) for x in docs]
    cum = np.concatenate([[0], np.cumsum([len(w) for w in want])])
    with mbpe.Decoder(m) as d:
        rc, b, n, bad = _batch(d, t, off)
        assert (rc, n, bad) == (0, int(cum[-1]), 0) and b.tolist() == cum.tolist()
        assert d.decode_batch(docs) == want
        # no documents and no tokens; only empty documents and no tokens: no kernel runs, every offset is 0
        rc, b, n, bad = _batch(d, [], [0])
        assert (rc, n, bad) == (0, 0, 0) and b.tolist() == [0]
        rc, b, n, bad = _batch(d, [], [0, 0, 0, 0])
        assert (rc, n, bad) == (0, 0, 0) and b.tolist() == [0, 0, 0, 0]
        assert d.decode_batch([], with_invalid=True) == ([], 0)
        assert d.decode_batch([[], [], []]) == [b"", b"", b""]
        # the offsets are checked before the device
        for wrong in ([0, 5, 4, 1500], [1, 1500], [0, 1499], [0, 1501]):
            assert _batch(d, t, wrong)[0] == mbpe.ERR_ARG, wrong
        assert _batch(d, [], [0, 1])[0] == mbpe.ERR_ARG
        assert _batch(d, t, [0, 1500], bits=8)[0] == mbpe.ERR_ARG


# ---- 4. the query and a cap one byte short --------------------------------------------------------------------------

def test_query_and_short_cap_still_fill_the_offsets():
    m = _golden_merges("shakespeare_basic_lexical_512")
    tok = _host_tok(m)
    t = np.ascontiguousarray(tok.encode(read_data("small.txt")), dtype=np.uint32)
    off = [0, 0, 1, len(t) // 3, len(t) // 3, len(t) - 1, len(t)]
    want = [tok.decode(t[lo:hi]) for lo, hi in zip(off[:-1], off[1:])]
    cum = np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist()
    total = cum[-1]
    with mbpe.Decoder(m) as d:
        rc, b, n, bad = _batch(d, t, off)                                    # bytes_out NULL
        assert (rc, n, bad) == (0, total, 0) and b.tolist() == cum
        out = np.full(total + 8, 0xAB, dtype=np.uint8)
        rc, b, n, bad = _batch(d, t, off, out, total - 1)
        assert rc == mbpe.ERR_ARG and (n, bad) == (total, 0) and b.tolist() == cum
        assert bool((out == 0xAB).all())
        rc, b, n, bad = _batch(d, t, off, out, total)
        assert (rc, n) == (0, total) and b.tolist() == cum
        assert out[:total].tobytes() == b"".join(want) and bool((out[total:] == 0xAB).all())


# ---- 5. offsets beyond 2^32 -----------------------------------------------------------------------------------------

def test_offsets_beyond_4_gib_query_only(dev):
    # 22 doublings of one byte: 2^0 (the byte itself), 2^1 (id 256), ..., 2^21 (id 276, the 21st merge).  One more merge
    # would make 2^22 bytes, beyond MBPE_DECODER_MAX_ENTRY.
    m = _doubling(21)
    top, ln = 256 + len(m) - 1, 1 << 21
    assert len(_host_tok(m).decode([top])) == ln
    t = torch.full((2500,), top, dtype=torch.int32, device=dev)
    off = [0, 2047, 2048, 2049, 2500]
    with mbpe.Decoder(m) as d:
        b, n, bad = d.decode_batch_device(t.data_ptr(), 2500, off, 0, 0)
    assert (n, bad) == (2500 * ln, 0) and n > (1 << 32)
    assert b.tolist() == [x * ln for x in off] and int(b[1]) < (1 << 32) <= int(b[2])


# ---- 6. plain 16-bit ids --------------------------------------------------------------------------------------------

def test_plain_16_bit_ids_and_the_old_hole(dev):
    # 65,280 merges of two raw bytes each: 65,536 entries, the last one (id 65,535) reads "Zq"
    m = np.array([[k >> 8, k & 255] for k in range(65279)] + [[ord("Z"), ord("q")]], dtype=np.uint32)
    assert 256 + len(m) == 65536
    tok = _host_tok(m)
    rng = np.random.default_rng(16)
    t = rng.integers(0, 65536, size=3000, dtype=np.uint32)
    t[[0, 7, 1023, 1024, 2999]] = 65535
    off = [0, 1, 1024, 2999, 3000]
    want = [tok.decode(t[lo:hi]) for lo, hi in zip(off[:-1], off[1:])]
    assert want[0] == b"Zq" and want[3] == b"Zq"
    cum = np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist()
    t16 = t.astype(np.uint16)
    with mbpe.Decoder(m) as d:
        # host tokens
        out = np.zeros(cum[-1], dtype=np.uint8)
        rc, b, n, bad = _batch(d, t16, off, out, len(out), bits=16)
        assert (rc, n, bad) == (0, cum[-1], 0) and b.tolist() == cum and out.tobytes() == b"".join(want)
        assert d.decode_batch([t16[lo:hi] for lo, hi in zip(off[:-1], off[1:])], dtype=np.uint16) == want
        # device tokens
        td = torch.from_numpy(t16.view(np.int16)).to(dev)
        buf = torch.zeros(cum[-1], dtype=torch.uint8, device=dev)
        b, n, bad = d.decode_batch_device(td.data_ptr(), len(t), off, buf.data_ptr(), cum[-1], token_bits=16)
        assert (n, bad) == (cum[-1], 0) and b.tolist() == cum
        assert buf.cpu().numpy().tobytes() == b"".join(want)
        # the same array as 16-bit slots: 0xFFFF stays a hole there
        holes = tok.decode(t[t != 65535])
        assert len(holes) == cum[-1] - 2 * int((t == 65535).sum()) < cum[-1] - 8
        n, bad = d.decode_slots_device(td.data_ptr(), len(t), 16, 0, None, buf.data_ptr(), cum[-1])
        assert (n, bad) == (len(holes), 0)
        assert buf[:n].cpu().numpy().tobytes() == holes


# ---- 7. encode -> decode on the device ------------------------------------------------------------------------------

def test_round_trip_on_the_device_with_16_bit_ids(dev):
    data = read_data("shakespeare.txt")
    merges = _golden_merges("shakespeare_gpt4_lexical_512")
    chunk_off = mbpe.presplit(O.GPT4_SPLIT_PATTERN, data).astype(np.uint64)
    text = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to(dev)
    tokens = torch.zeros(len(data), dtype=torch.int16, device=dev)
    out = torch.zeros(len(data) + 16, dtype=torch.uint8, device=dev)
    with mbpe.Encoder(merges) as e, mbpe.Decoder(merges) as d:
        n_tok, tok_off = e.encode_device(text.data_ptr(), len(data), chunk_off, tokens.data_ptr(), len(data),
                                         token_bits=16, offsets=True)
        assert 0 < n_tok < len(data) and int(tok_off[-1]) == n_tok
        b, n, bad = d.decode_batch_device(tokens.data_ptr(), n_tok, tok_off, out.data_ptr(), len(data), token_bits=16)
        assert d.kernel_ms() > 0
    assert (n, bad) == (len(data), 0)
    assert np.array_equal(b, chunk_off)
    assert bool(torch.equal(out[:len(data)], text)) and int(out[len(data):].sum()) == 0


# ---- 8. the offset arrays are kept ----------------------------------------------------------------------------------

def test_a_repeat_call_allocates_nothing():
    m = _golden_merges("shakespeare_basic_lexical_512")
    tok = _host_tok(m)
    t = np.ascontiguousarray(tok.encode(read_data("sample.txt")), dtype=np.uint32)
    off = np.linspace(0, len(t), 40).astype(np.uint64)
    want = tok.decode(t)
    with mbpe.Decoder(m) as d:
        a0 = d.alloc_count()
        assert a0 > 0
        out1, out2 = np.zeros(len(want), dtype=np.uint8), np.zeros(len(want), dtype=np.uint8)
        r1 = _batch(d, t, off, out1, len(want))
        a1 = d.alloc_count()
        r2 = _batch(d, t, off, out2, len(want))
        assert a1 > a0 and d.alloc_count() == a1
        assert r1[0] == r2[0] == 0 and r1[2:] == r2[2:] == (len(want), 0) and np.array_equal(r1[1], r2[1])
        assert out1.tobytes() == out2.tobytes() == want
        # smaller: fewer tokens, fewer documents
        k = len(t) // 2
        assert k >= 4
        r3 = _batch(d, t[:k], [0, k // 2, k], out2, len(want))
        assert r3[0] == 0 and d.alloc_count() == a1
        assert out2[:r3[2]].tobytes() == tok.decode(t[:k]) and int(r3[1][1]) == len(tok.decode(t[:k // 2]))
