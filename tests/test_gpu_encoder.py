"""The persistent device encoder (mbpe_encoder_*, mbpe.Encoder, Tokenizer.encode_batch) on the GPU.

The judge is oracle.encode_chunks chunk by chunk (oracle_encode of tests/test_gpu_encode_spans.py: the per-chunk
lengths of the oracle give the expected chunk offsets) and the one-shot mbpe.encode_chunks.  The cases come from
tests/encode_cases.py.  Every comparison is on whole arrays."""
import ctypes

import numpy as np
import pytest

import mbpe
import oracle as O
import encode_cases as E
from conftest import read_data
from test_gpu_encode_spans import _same, oracle_encode
from test_tokenizer_cpu import _golden_merges

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

END = 0x80000000


@pytest.fixture(scope="module")
def dev():
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def _n_chunks(c):
    return 1 if c.chunk_off is None else len(c.chunk_off) - 1


def _prefix(c):
    """About the first half of a case, cut at a chunk boundary."""
    if c.chunk_off is None:
        return E.Case(np.ascontiguousarray(c.data[:len(c.data) // 2]), None, c.merges, c.name + " (first half)")
    k = max(_n_chunks(c) // 2, 1)
    off = np.ascontiguousarray(c.chunk_off[:k + 1])
    return E.Case(np.ascontiguousarray(c.data[:int(off[-1])]), off, c.merges, c.name + " (first %d chunks)" % k)


def _expect(c):
    want, lens = oracle_encode(c)
    return want, np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)


def _check_case(enc, c, expect=None):
    """One call of the encoder against the oracle and the one-shot call: tokens, count, passes, chunk offsets."""
    want, want_off = expect or _expect(c)
    one, one_passes = mbpe.encode_chunks(c.data, c.chunk_off, c.merges)
    _same(one, want, one_passes, c.name + " (one-shot)")
    got, off = enc.encode(c.data, c.chunk_off, offsets=True)
    _same(got, want, enc.n_passes, c.name + " (encoder)")
    assert enc.n_passes == one_passes, (c.name, enc.n_passes, one_passes)
    assert off.dtype == np.uint64 and len(off) == _n_chunks(c) + 1, c.name
    if not np.array_equal(off, want_off):
        at = int(np.flatnonzero(off != want_off)[0])
        pytest.fail("%s: chunk_tok_off[%d] = %d, want %d" % (c.name, at, off[at], want_off[at]))
    assert off[0] == 0 and off[-1] == len(got), c.name
    plain = enc.encode(c.data, c.chunk_off)                       # without the end list: the same tokens
    _same(plain, want, enc.n_passes, c.name + " (encoder, no offsets)")
    return got, off


def _groups():
    cases = [E.fuzz_case(np.random.default_rng(4200 + s)) for s in range(4)]
    cases += E.nul_cases(np.random.default_rng(4300))
    cases += E.lookup_cases()
    groups = {}
    for c in cases:
        groups.setdefault(np.ascontiguousarray(c.merges, dtype=np.uint32).tobytes(), []).append(c)
    return list(groups.values())


def test_one_encoder_many_texts():
    """Per merges table ONE encoder: the largest case, a prefix of it and the other cases (smaller), the largest again.
    Buffers that keep an earlier call's content beyond the new length would show."""
    groups = _groups()
    assert len(groups) >= 4 + 1 + 7 - 1                         # fuzz tables, the NUL table, the lookup tables
    for g in groups:
        g = sorted(g, key=lambda c: len(c.data))
        large = g[-1]
        expect = _expect(large)
        with mbpe.Encoder(large.merges) as enc:
            _check_case(enc, large, expect)
            for c in [_prefix(large)] + g[:-1]:
                _check_case(enc, c)
            _check_case(enc, large, expect)


def _handmade():
    """Empty chunks first, last and three in a row, NUL-led single chunks first and last (of the chunks that are not
    empty), chunk ends on a span edge and next to the slice edges (more than 1,024 spans: two spans per slice)."""
    n_body = (E.SLICES + E.SLICES // 2) * E.SPAN + 5
    head, tail = b"\x00300", b"\x007"
    body = np.tile(np.frombuffer(b"ab", dtype=np.uint8), n_body // 2 + 1)[:n_body]
    data = np.concatenate([np.frombuffer(head, dtype=np.uint8), body, np.frombuffer(tail, dtype=np.uint8)])
    n = len(data)
    cuts = [len(head), n - len(tail), 3 * E.SPAN, 7 * E.SPAN, 7 * E.SPAN + 1]
    for rot in range(3):
        cuts += E.slice_edge_cuts(n, E.SPAN, E.SLICES, rot)
    cuts = sorted(set(c for c in cuts if len(head) <= c <= n - len(tail)))
    mid = cuts[len(cuts) // 2]
    off = [0, 0] + cuts[:cuts.index(mid) + 1] + [mid, mid, mid] + cuts[cuts.index(mid) + 1:] + [n, n]
    off = np.array(off, dtype=np.uint64)
    assert off[0] == off[1] == 0 and off[-1] == off[-2] == n and (np.diff(off.astype(np.int64)) >= 0).all()
    merges = np.concatenate([E.run_merges(), np.array([[300, 97], [98, 7], [278, 278]], dtype=np.uint32)])
    return E.Case(np.ascontiguousarray(data), off, merges, "handmade: empty chunks, NUL-led ends, span and slice edges")


def test_chunk_offsets():
    c = _handmade()
    want, want_off = _expect(c)
    lens = np.diff(want_off.astype(np.int64))
    assert lens[0] == 0 and lens[1] == 1 and lens[-1] == 0 and lens[-2] == 1 and (lens == 0).sum() >= 5
    assert want[0] == 300 and want[-1] == 7
    with mbpe.Encoder(c.merges) as enc:
        got, off = _check_case(enc, c, (want, want_off))
        # chunk by chunk against the oracle's own chunk
        text = np.ascontiguousarray(c.data)
        for k in range(_n_chunks(c)):
            s, e = int(c.chunk_off[k]), int(c.chunk_off[k + 1])
            chunk = O.encode_chunks(text[s:e], None, c.merges) if e > s else np.zeros(0, dtype=np.uint32)
            assert np.array_equal(got[int(off[k]):int(off[k + 1])], chunk), (k, s, e)
        # a query reports the offsets too
        rc, n, passes, _, off_q = _raw(enc, c.data, c.chunk_off, out=False, offsets=True)
        assert rc == mbpe.OK and n == len(want) and np.array_equal(off_q, want_off)


def one_byte_chunks():
    """Every byte a chunk of its own, three spans and five bytes of them: nothing merges, and the list of chunk ends
    (8 bytes per chunk) is twice the size of a token array (4 bytes per byte), so a fresh encoder, whose buffers hold
    exactly what the call asks for, cannot keep the list in the idle token array and gives it a buffer of its own."""
    n = 3 * E.SPAN + 5
    data = np.ascontiguousarray(np.tile(np.frombuffer(b"ab", dtype=np.uint8), n // 2 + 1)[:n])
    merges = np.array([[97, 98], [256, 256]], dtype=np.uint32)
    return E.Case(data, np.arange(n + 1, dtype=np.uint64), merges, "one-byte chunks")


def test_chunk_offsets_of_one_byte_chunks():
    c = one_byte_chunks()
    want, want_off = _expect(c)
    assert np.array_equal(want, O.encode_chunks(c.data, c.chunk_off, c.merges))
    assert np.array_equal(want, c.data) and np.array_equal(want_off, c.chunk_off)     # (what the oracle says of it)
    h = _handmade()
    with mbpe.Encoder(c.merges) as enc:
        got, off = enc.encode(c.data, c.chunk_off, offsets=True)
        _same(got, want, enc.n_passes, c.name)
        assert off.dtype == np.uint64 and np.array_equal(off, want_off)
        got16, off16 = enc.encode(c.data, c.chunk_off, offsets=True, dtype=np.uint16)
        assert got16.dtype == np.uint16 and np.array_equal(got16, want.astype(np.uint16))
        assert np.array_equal(off16, want_off)
        # the same encoder afterwards on the ordinary path: the spill leaves it intact
        _check_case(enc, E.Case(h.data, h.chunk_off, c.merges, h.name + " (after one-byte chunks)"))


# ---- the C function as it is --------------------------------------------------------------------------------------

def _raw(enc, data, off=None, cap=None, out=True, bits=32, offsets=False):
    text = np.ascontiguousarray(np.frombuffer(bytes(data), dtype=np.uint8) if isinstance(data, bytes) else data)
    off = None if off is None else np.ascontiguousarray(off, dtype=np.uint64)
    n_chunks = 1 if off is None else len(off) - 1
    cap = max(len(text), 1) if cap is None else cap
    buf = np.full((min(cap, len(text) + 8) if out else 0) + 2, 0xABABABAB, dtype=np.uint32)
    tok_off = np.full(n_chunks + 1, 0x5555555555555555, dtype=np.uint64) if offsets else None
    n, passes = ctypes.c_uint64(77), ctypes.c_uint32(77)
    rc = mbpe.lib().mbpe_encoder_encode(
        enc._h, text.ctypes.data if len(text) else None, len(text), 0, None if off is None else off.ctypes.data,
        0 if off is None else n_chunks, buf.ctypes.data if out else None, cap, bits, 0,
        None if tok_off is None else tok_off.ctypes.data, ctypes.byref(n), ctypes.byref(passes))
    return rc, n.value, passes.value, buf, tok_off


MERGES = np.array([[97, 98], [256, 99], [257, 257]], dtype=np.uint32)
TEXT = b"abcabcab" * 300 + b"c"


def test_query_and_capacity():
    want = O.encode_chunks(TEXT, None, MERGES)
    with mbpe.Encoder(MERGES) as enc:
        rc, n, passes, buf, _ = _raw(enc, TEXT, cap=len(want))
        assert (rc, n, passes) == (mbpe.OK, len(want), 4) and np.array_equal(buf[:n], want)
        assert (buf[n:] == 0xABABABAB).all()
        for cap in (0, 5, 1 << 40):                                  # NULL output: the count, whatever cap says
            assert _raw(enc, TEXT, cap=cap, out=False)[:3] == (mbpe.OK, len(want), 4)
        rc, n, passes, buf, off = _raw(enc, TEXT, cap=len(want) - 1, offsets=True)
        assert (rc, n, passes) == (mbpe.ERR_ARG, len(want), 4) and (buf == 0xABABABAB).all()
        assert b"too small" in mbpe.lib().mbpe_last_error()
        # 16-bit output is counted in tokens as well
        rc, n, passes, buf, _ = _raw(enc, TEXT, cap=len(want) - 1, bits=16)
        assert (rc, n) == (mbpe.ERR_ARG, len(want)) and (buf == 0xABABABAB).all()
        # an empty text, with and without chunks
        assert _raw(enc, b"")[:3] == (mbpe.OK, 0, 0)
        rc, n, passes, _, off = _raw(enc, b"", np.array([0, 0, 0, 0], dtype=np.uint64), offsets=True)
        assert (rc, n, passes) == (mbpe.OK, 0, 0) and off.tolist() == [0, 0, 0, 0]
        toks, off = enc.encode(b"", None, offsets=True)
        assert len(toks) == 0 and off.tolist() == [0, 0]
        # chunk offsets are checked as in the one-shot call
        for bad in ([0, 9, 6, len(TEXT)], [0, 6, len(TEXT) - 1], [1, 6, len(TEXT)]):
            assert _raw(enc, TEXT, np.array(bad, dtype=np.uint64))[:3] == (mbpe.ERR_ARG, 0, 0), bad
        # and the encoder still works
        assert np.array_equal(enc.encode(TEXT), want)


def test_token_bits_and_option_names():
    want = O.encode_chunks(TEXT, None, MERGES)
    with mbpe.Encoder(MERGES) as enc:
        for bits in (0, 8, 24, 31, 64):
            rc, n, passes, buf, _ = _raw(enc, TEXT, bits=bits)
            assert (rc, n, passes) == (mbpe.ERR_ARG, 0, 0) and (buf == 0xABABABAB).all(), bits
        with pytest.raises(mbpe.MbpeError) as e:
            enc.set_option("piece_byte", 4096)
        assert e.value.code == mbpe.ERR_ARG
        with pytest.raises(mbpe.MbpeError) as e:
            enc.set_option("piece_bytes", -1)
        assert e.value.code == mbpe.ERR_ARG
        with pytest.raises(ValueError):
            enc.encode(TEXT, dtype=np.uint8)
        assert np.array_equal(enc.encode(TEXT), want)
        assert enc.kernel_ms() > 0.0


# ---- device text, device output -------------------------------------------------------------------------------------

def _device_call(enc, c, dev, bits=32):
    """Text in a CUDA tensor, tokens into a CUDA tensor -> (raw slots as numpy, count, offsets); checks that the text
    tensor is bit-identical afterwards and nothing is written beyond the count."""
    data = np.ascontiguousarray(c.data)
    text = torch.from_numpy(data.copy()).to(dev)
    before = text.clone()
    out = torch.zeros(len(data) + 3, dtype=torch.int32 if bits == 32 else torch.int16, device=dev)
    n, off = enc.encode_device(text.data_ptr(), len(data), c.chunk_off, out.data_ptr(), out.numel(), bits, offsets=True)
    assert torch.equal(text, before), c.name + ": the text on the device was written"
    raw = out.cpu().numpy().view(np.uint32 if bits == 32 else np.uint16)
    assert not raw[n:].any(), c.name + ": tokens written beyond n_out"
    return raw[:n], n, off, out


def test_device_text_device_output(dev):
    cases = [E.fuzz_case(np.random.default_rng(4201))] + E.nul_cases(np.random.default_rng(4300))
    cases += [c for c in E.lookup_cases() if len(c.merges) == 50]
    for c in cases:
        with mbpe.Encoder(c.merges) as enc:
            host, host_off = enc.encode(c.data, c.chunk_off, offsets=True)
            passes = enc.n_passes
            _same(host, O.encode_chunks(c.data, c.chunk_off, c.merges), passes, c.name)
            raw, n, off, _ = _device_call(enc, c, dev)
            assert n == len(host) and enc.n_passes == passes, c.name
            _same(raw & np.uint32(END - 1), host, passes, c.name + " (device text, device output)")
            assert np.array_equal(off, host_off), c.name
            ends = np.zeros(n, dtype=bool)
            ends[np.unique(host_off[1:]).astype(np.int64)[np.unique(host_off[1:]) > 0] - 1] = True
            assert np.array_equal((raw & np.uint32(END)) != 0, ends), c.name + ": chunk-end flags"
            # device text, host output
            text = torch.from_numpy(np.ascontiguousarray(c.data).copy()).to(dev)
            buf = np.zeros(max(len(c.data), 1), dtype=np.uint32)
            cnt = ctypes.c_uint64()
            o = None if c.chunk_off is None else np.ascontiguousarray(c.chunk_off, dtype=np.uint64)
            rc = mbpe.lib().mbpe_encoder_encode(enc._h, ctypes.c_void_p(text.data_ptr()), len(c.data), 1,
                                                None if o is None else o.ctypes.data, 0 if o is None else len(o) - 1,
                                                buf.ctypes.data, len(buf), 32, 0, None, ctypes.byref(cnt), None)
            assert rc == mbpe.OK
            _same(buf[:cnt.value], host, passes, c.name + " (device text, host output)")


def test_device_text_nul_led_ids_the_device_refuses(dev):
    with mbpe.Encoder(E.nul_merges()) as enc:
        for c in E.nul_error_cases():
            assert _raw(enc, c.data, c.chunk_off)[:3] == (mbpe.ERR_ARG, 0, 0), c.name
            text = torch.from_numpy(np.ascontiguousarray(c.data).copy()).to(dev)
            out = torch.zeros(len(c.data), dtype=torch.int32, device=dev)
            with pytest.raises(mbpe.MbpeError) as e:
                enc.encode_device(text.data_ptr(), len(c.data), c.chunk_off, out.data_ptr(), out.numel())
            assert e.value.code == mbpe.ERR_ARG and not out.any(), c.name
        assert enc.encode(b"abcabc").tolist() == O.encode_chunks(b"abcabc", None, E.nul_merges()).tolist()


def test_device_output_decodes_back_to_the_text(dev):
    c = E.fuzz_case(np.random.default_rng(4202))
    with mbpe.Encoder(c.merges) as enc, mbpe.Decoder(c.merges) as dec:
        raw, n, off, out = _device_call(enc, c, dev)
        back = torch.zeros(len(c.data) + 1, dtype=torch.uint8, device=dev)
        n_bytes, bad = dec.decode_slots_device(out.data_ptr(), n, 32, END, None, back.data_ptr(), back.numel())
        assert (n_bytes, bad) == (len(c.data), 0)
        assert np.array_equal(back[:n_bytes].cpu().numpy(), np.ascontiguousarray(c.data))


# ---- 16-bit ids ---------------------------------------------------------------------------------------------------

def test_16_bit_output(dev):
    cases = [E.fuzz_case(np.random.default_rng(4203))]
    cases += [c for c in E.lookup_cases() if len(c.merges) in (8, (1 << 15) - 1)]
    for c in cases:
        with mbpe.Encoder(c.merges) as enc:
            wide, off = enc.encode(c.data, c.chunk_off, offsets=True)
            assert wide.max() < 65536
            narrow, off16 = enc.encode(c.data, c.chunk_off, offsets=True, dtype=np.uint16)
            assert narrow.dtype == np.uint16 and np.array_equal(narrow, wide.astype(np.uint16)), c.name
            assert np.array_equal(off, off16), c.name
            raw, n, off_dev, _ = _device_call(enc, c, dev, bits=16)
            assert raw.dtype == np.uint16 and np.array_equal(raw, wide.astype(np.uint16)), c.name   # ids without flags
            assert np.array_equal(off_dev, off), c.name


def test_16_bit_refuses_what_does_not_fit():
    text = b"ab" * 100
    for n_merges, fits in ((65281, False), (65280, True)):
        m = np.stack([np.arange(n_merges, dtype=np.uint32) + 1000, np.arange(n_merges, dtype=np.uint32) + 70000], axis=1)
        m[0] = (97, 98)
        m[-1] = (256, 256)
        with mbpe.Encoder(m) as enc:
            wide = enc.encode(text)
            assert wide.tolist() == [256 + n_merges - 1] * 50
            if fits:
                assert enc.encode(text, dtype=np.uint16).tolist() == wide.tolist()
                continue
            rc, n, passes, buf, _ = _raw(enc, text, bits=16)
            assert (rc, n, passes) == (mbpe.ERR_VOCAB, 0, 0) and (buf == 0xABABABAB).all()
            assert np.array_equal(enc.encode(text), wide)                # the encoder works afterwards
    m = np.array([[97, 98]], dtype=np.uint32)
    with mbpe.Encoder(m) as enc:
        for marker, fits in ((b"\x0065535", True), (b"\x0065536", False), (b"\x00 +70000", False)):
            data = b"abab" + marker + b"ab"
            off = np.array([0, 4, 4 + len(marker), len(data)], dtype=np.uint64)
            wide = enc.encode(data, off)
            assert wide.tolist() == [256, 256, int(marker[1:]), 256]
            if fits:
                assert enc.encode(data, off, dtype=np.uint16).tolist() == wide.tolist()
                continue
            rc, n, passes, buf, _ = _raw(enc, data, off, bits=16)
            assert (rc, n, passes) == (mbpe.ERR_VOCAB, 0, 0) and (buf == 0xABABABAB).all(), marker
            assert np.array_equal(enc.encode(data, off), wide)


# ---- pieces -------------------------------------------------------------------------------------------------------

def _pieces(off, limit):
    """The cut mbpe.h describes: every piece takes as many whole chunks as fit into `limit` bytes."""
    off = [int(o) for o in off]
    out, c0 = [], 0
    while c0 < len(off) - 1:
        c1 = c0
        while c1 < len(off) - 1 and off[c1 + 1] - off[c0] <= limit:
            c1 += 1
        assert c1 > c0
        out.append((c0, c1))
        c0 = c1
    return out


def test_pieces():
    rng = np.random.default_rng(77001)
    train = np.repeat(rng.integers(97, 101, size=4000, dtype=np.uint8), rng.integers(1, 6, size=4000))
    merges, _ = O.train(np.ascontiguousarray(train), 256 + 200)
    n = 1 << 20
    data = np.ascontiguousarray(np.repeat(rng.integers(97, 101, size=n, dtype=np.uint8), rng.integers(1, 6, size=n))[:n])
    cuts = np.unique(rng.integers(1, n, size=n // 40))
    off = np.concatenate([[0], cuts, [n]]).astype(np.uint64)
    assert n / (len(off) - 1) <= 50
    limit = 65536
    pieces = _pieces(off, limit)
    assert len(pieces) >= 16
    c = E.Case(data, off, merges, "pieces")
    want, want_off = _expect(c)
    with mbpe.Encoder(merges) as enc:
        whole, whole_off = enc.encode(data, off, offsets=True)
        _same(whole, want, enc.n_passes, "unsplit")
        assert np.array_equal(whole_off, want_off)
        deepest = 0
        for c0, c1 in pieces:                                   # every piece alone
            s, e = int(off[c0]), int(off[c1])
            got = enc.encode(data[s:e], off[c0:c1 + 1] - off[c0])
            assert np.array_equal(got, whole[int(whole_off[c0]):int(whole_off[c1])])
            deepest = max(deepest, enc.n_passes)
        enc.set_option("piece_bytes", limit)
        got, got_off = enc.encode(data, off, offsets=True)
        _same(got, whole, enc.n_passes, "in %d pieces" % len(pieces))
        assert np.array_equal(got_off, whole_off)
        assert enc.n_passes == deepest
        assert np.array_equal(enc.encode(data, off, dtype=np.uint16), whole.astype(np.uint16))
        # an output with room for exactly the tokens (less than n_bytes: the count runs first), and for one less
        rc, cnt, passes, buf, off_raw = _raw(enc, data, off, cap=len(whole), offsets=True)
        assert (rc, cnt, passes) == (mbpe.OK, len(whole), deepest)
        assert np.array_equal(buf[:cnt], whole) and (buf[cnt:] == 0xABABABAB).all() and np.array_equal(off_raw, whole_off)
        rc, cnt, passes, buf, _ = _raw(enc, data, off, cap=len(whole) - 1)
        assert (rc, cnt, passes) == (mbpe.ERR_ARG, len(whole), deepest) and (buf == 0xABABABAB).all()
        # the same text as ONE chunk does not fit a piece
        rc, cnt, passes, buf, _ = _raw(enc, data, None)
        assert (rc, cnt, passes) == (mbpe.ERR_OOM, 0, 0) and (buf == 0xABABABAB).all()
        msg = mbpe.lib().mbpe_last_error()
        assert b"chunk 0" in msg and b"1048576" in msg and b"piece_bytes" in msg, msg
        enc.set_option("piece_bytes", 0)
        one = enc.encode(data, None)
        assert np.array_equal(one, O.encode_chunks(data, None, merges))
        # piece_bytes exactly the longest chunk's length
        longest = int(np.diff(off.astype(np.int64)).max())
        enc.set_option("piece_bytes", longest)
        got, got_off = enc.encode(data, off, offsets=True)
        assert np.array_equal(got, whole) and np.array_equal(got_off, whole_off)
        enc.set_option("piece_bytes", longest - 1)
        assert _raw(enc, data, off)[0] == mbpe.ERR_OOM


def test_pieces_of_a_device_text(dev):
    """Pieces with the text and the output on the device, NUL-led chunks included: every piece scans its own chunk
    starts and writes behind the one before it."""
    cases = [c for c in E.nul_cases(np.random.default_rng(4300)) if "random mixture" in c.name]
    assert len(cases) == 1
    c = cases[0]
    with mbpe.Encoder(c.merges) as enc:
        raw0, n0, off0, _ = _device_call(enc, c, dev)
        enc.set_option("piece_bytes", 2048)
        assert len(_pieces(c.chunk_off, 2048)) >= 8
        raw, n, off, _ = _device_call(enc, c, dev)
        assert n == n0 and np.array_equal(raw, raw0) and np.array_equal(off, off0)
        _same(raw & np.uint32(END - 1), O.encode_chunks(c.data, c.chunk_off, c.merges), enc.n_passes, c.name)


# ---- reuse --------------------------------------------------------------------------------------------------------

def test_reuse_is_real():
    c = E.fuzz_case(np.random.default_rng(4200))
    small = _prefix(c)
    larger = E.Case(np.concatenate([c.data, c.data[:4096]]), None, c.merges, "larger")
    with mbpe.Encoder(c.merges) as enc:
        a0 = enc.alloc_count()
        assert a0 >= 1                                            # the lookup table
        first = enc.encode(c.data, c.chunk_off, offsets=True)[0]
        a1 = enc.alloc_count()
        assert a1 > a0
        enc.encode(small.data, small.chunk_off, offsets=True)
        assert enc.alloc_count() == a1                            # a text no larger: no allocation
        again = enc.encode(c.data, c.chunk_off, offsets=True)[0]
        assert enc.alloc_count() == a1 and np.array_equal(first, again)
        enc.encode(c.data, c.chunk_off, dtype=np.uint16)
        assert enc.alloc_count() == a1                            # the 16-bit output goes through the same buffers
        enc.encode(larger.data, None)
        assert enc.alloc_count() > a1                             # a larger text: the buffers grow


# ---- Tokenizer ----------------------------------------------------------------------------------------------------

def test_tokenizer_keeps_and_drops_its_encoder():
    data = read_data("sample.txt")
    tok = mbpe.Tokenizer("")
    tok.set_merges(_golden_merges("shakespeare_basic_lexical_512"))
    host = tok.encode(data)
    assert np.array_equal(tok.encode(data, device=0), host)
    assert np.array_equal(tok.encode(data[:1000], device=0), tok.encode(data[:1000]))
    assert np.array_equal(tok.encode(data, device=0), host)
    tok.set_merges(_golden_merges("taylorswift_basic_lexical_512"))         # a stale encoder would show
    host2 = tok.encode(data)
    assert not np.array_equal(host2, host)
    assert np.array_equal(tok.encode(data, device=0), host2)
    # special tokens do not enter the table: changing them alone keeps the encoder, and the results follow them
    tok.set_special_tokens_from_file(b"<|x|> 70000\n")
    text = data[:500] + b"<|x|>" + data[500:900]
    assert np.array_equal(tok.encode(text, device=0), tok.encode(text))
    assert 70000 in tok.encode(text, device=0).tolist()
    tok.close()


def _batch_check(tok, texts):
    got = tok.encode_batch(texts, device=0)
    assert len(got) == len(texts)
    for i, (g, t) in enumerate(zip(got, texts)):
        assert g.dtype == np.uint32 and np.array_equal(g, tok.encode(t)), (i, t[:40])
    return got


def test_tokenizer_encode_batch():
    tok = mbpe.Tokenizer(O.GPT4_SPLIT_PATTERN)
    tok.set_special_tokens_from_file(read_data("special1.txt"))
    tok.set_merges(_golden_merges("taylorswift_gpt4_first_512"))
    sample = read_data("specialtokensample.txt")
    _batch_check(tok, [sample])
    _batch_check(tok, [sample, b"", sample[:20], sample[5:], b""])
    tok.close()
    tok = mbpe.Tokenizer(O.GPT4_SPLIT_PATTERN)
    tok.set_merges(_golden_merges("taylorswift_gpt4_lexical_512"))
    data = read_data("taylorswift.txt")
    lines = data.splitlines(keepends=True)
    assert len(lines) > 100 and b"".join(lines) == data
    got = _batch_check(tok, lines)
    _batch_check(tok, [b"", b"", lines[0], b"", lines[1], b""])
    assert [len(g) for g in tok.encode_batch([b"", b""], device=0)] == [0, 0]
    assert tok.encode_batch([], device=0) == []
    # the C function: the same flat array and offsets
    doc_off = np.concatenate([[0], np.cumsum([len(x) for x in lines])]).astype(np.uint64)
    text = np.frombuffer(data, dtype=np.uint8)
    n = ctypes.c_uint64()
    L = mbpe.lib()
    assert L.mbpe_tok_encode_batch_device(tok._h, text.ctypes.data, doc_off.ctypes.data, len(lines), 0, 0, None, 0, None,
                                          ctypes.byref(n)) == mbpe.OK
    flat_want = np.concatenate(got)
    assert n.value == len(flat_want)
    out = np.zeros(n.value, dtype=np.uint32)
    tok_off = np.zeros(len(lines) + 1, dtype=np.uint64)
    assert L.mbpe_tok_encode_batch_device(tok._h, text.ctypes.data, doc_off.ctypes.data, len(lines), 0, 0,
                                          out.ctypes.data, len(out), tok_off.ctypes.data, ctypes.byref(n)) == mbpe.OK
    assert np.array_equal(out, flat_want)
    assert np.array_equal(tok_off, np.concatenate([[0], np.cumsum([len(g) for g in got])]).astype(np.uint64))
    small = np.zeros(n.value - 1, dtype=np.uint32)
    assert L.mbpe_tok_encode_batch_device(tok._h, text.ctypes.data, doc_off.ctypes.data, len(lines), 0, 0,
                                          small.ctypes.data, len(small), None, ctypes.byref(n)) == mbpe.ERR_ARG
    assert n.value == len(flat_want) and not small.any()
    tok.close()
