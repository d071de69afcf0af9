"""Encode on the device (csrc/encode.hip) past 1,024 spans, with full spans, NUL-led chunks across every edge, lookup
tables whose chains wrap, the C-ABI's edges and a text beyond 2^32 bytes.

The passes cut the token array into spans of 1,024 tokens and link them with two single-workgroup scans of 1,024
threads (k_enc_scan_parity, k_enc_scan_sum); thread t owns per = ceil(n_spans / 1,024) consecutive spans.
tests/test_gpu_encode.py reaches per > 1 only with text in which no span is full.  The cases come from
tests/encode_cases.py; the judge is oracle.encode_chunks, which tests/test_encode_cases_cpu.py ties to a brute-force
encode on the same shapes at 1/32 of the size.  Every case is compared whole: np.array_equal on all tokens."""
import ctypes
import time

import numpy as np
import pytest

import mbpe
import oracle as O
import encode_cases as E
from test_encode_cases_cpu import SCALE, brute_force_chunks

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

END = 0x80000000


@pytest.fixture(scope="module")
def dev():
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def oracle_encode(case):
    """oracle.encode_chunks, and the number of tokens every chunk became."""
    text = np.ascontiguousarray(case.data, dtype=np.uint8)
    merges = np.ascontiguousarray(case.merges, dtype=np.uint32)
    off = [0, len(text)] if case.chunk_off is None else [int(o) for o in case.chunk_off]
    lib = O.lib()
    enc = lib.orc_encoder_new(merges.ctypes.data, len(merges))
    out, lens = [], []
    try:
        for s, e in zip(off[:-1], off[1:]):
            buf = np.zeros(max(e - s, 1), dtype=np.uint32)
            seg = text[s:e]
            n = lib.orc_text_to_vector(seg.ctypes.data if e > s else None, e - s, buf.ctypes.data)
            n = lib.orc_encode_chunk(enc, buf.ctypes.data, n)
            out.append(buf[:n].copy())
            lens.append(int(n))
    finally:
        lib.orc_encoder_free(enc)
    return (np.concatenate(out) if out else np.zeros(0, dtype=np.uint32)), np.array(lens, dtype=np.int64)


def _same(got, want, passes, name):
    if np.array_equal(got, want):
        return
    n = min(len(got), len(want))
    d = np.flatnonzero(got[:n] != want[:n])
    at = int(d[0]) if len(d) else n
    pytest.fail("%s: %d tokens, want %d; first difference at output index %d (got %s, want %s) after %d passes.  "
                "Output index // 1024 = %d is a span of the LAST pass only: the cause lies in an earlier pass at a "
                "position further right by the tokens merged away before it." % (
                    name, len(got), len(want), at, got[at:at + 4].tolist(), want[at:at + 4].tolist(), passes, at // 1024))


def _check(case, dev, passes_want=None):
    want, lens = oracle_encode(case)
    assert np.array_equal(want, O.encode_chunks(case.data, case.chunk_off, case.merges))
    got, passes = mbpe.encode_chunks(case.data, case.chunk_off, case.merges)
    _same(got, want, passes, case.name)
    if passes_want is not None:
        assert passes == passes_want, (case.name, passes, passes_want)
    # the result left on the device: the same ids, bit 31 on exactly the last token of every chunk that is not empty
    buf = torch.zeros(max(len(want), 1) + 3, dtype=torch.int32, device=dev)
    n, passes_dev = mbpe.encode_chunks_device(case.data, case.chunk_off, case.merges, buf.data_ptr(), buf.numel())
    raw = buf.cpu().numpy().view(np.uint32)
    assert n == len(want) and passes_dev == passes, case.name
    assert not raw[n:].any(), case.name + ": tokens written beyond n_out"
    _same(raw[:n] & np.uint32(END - 1), want, passes, case.name + " (left on the device)")
    want_ends = np.zeros(n, dtype=bool)
    want_ends[np.cumsum(lens[lens > 0]) - 1] = True
    ends = (raw[:n] & np.uint32(END)) != 0
    if not np.array_equal(ends, want_ends):
        at = int(np.flatnonzero(ends != want_ends)[0])
        pytest.fail("%s: chunk-end flag differs first at token %d (got %d, want %d), %d passes" % (
            case.name, at, ends[at], want_ends[at], passes))
    return passes


# ---- the cases of tests/encode_cases.py at full size ----------------------------------------------------------------

@pytest.fixture(scope="module")
def runs():
    return E.run_cases()


@pytest.mark.parametrize("which", range(len(E.N_SPANS)), ids=["n_spans=%d*1024%+d" % ab for ab in E.N_SPANS])
def test_runs_and_periods_across_slices(runs, dev, which):
    mine = runs[12 * which:12 * which + 12]
    a, b = E.N_SPANS[which]
    assert len(mine) == 12 and all(-(-len(c.data) // E.SPAN) == a * E.SLICES + b for c in mine)
    for c in mine:
        _check(c, dev)


def test_span_count_shrinks_from_three_per_slice_to_one(runs, dev):
    """5 Mi + 1 bytes of one letter: 5,121 spans in the first pass (per = 6), 2,561 in the second (3), 1,281 in the
    third (2), 641 in the fourth (1): the span arrays keep the earlier passes' values beyond the new n_spans."""
    c = [c for c in runs if c.name.startswith("run:a ") and c.chunk_off is None][-1]
    assert -(-len(c.data) // E.SPAN) == 5 * E.SLICES + 1
    assert _check(c, dev) >= 5                                   # (a pass halves the run at best)


@pytest.mark.parametrize("seed", range(4))
def test_fuzz_at_megabytes(dev, seed):
    c = E.fuzz_case(np.random.default_rng(4200 + seed))
    assert len(c.data) >= 1 << 20
    _check(c, dev)


def test_nul_led_chunks_across_groups_spans_and_slices(dev):
    for c in E.nul_cases(np.random.default_rng(4300)):
        _check(c, dev)
        if c.tok is not None:
            # the same chunks reached through a Tokenizer: host splitter -> markers -> device
            text, specials = c.tok
            t = mbpe.Tokenizer("")
            t.set_special_tokens_from_file(specials)
            t.set_merges(c.merges)
            on_device, on_host = t.encode(text, device=0), t.encode(text)
            _same(on_device, on_host, -1, c.name + " (Tokenizer, device against host)")
            _same(on_device, O.encode_chunks(c.data, c.chunk_off, c.merges), -1, c.name + " (Tokenizer against the oracle)")
            t.close()


def test_nul_led_ids_the_device_refuses():
    """mbpe.h: token ids must stay below 2^31 - 2.  A NUL-led chunk that names 0x7FFFFFFE, 0x7FFFFFFF or a negative
    value is MBPE_ERR_ARG on the device (and a token on the host: tests/test_encode_cases_cpu.py)."""
    for c in E.nul_error_cases():
        rc, n_out, passes, _ = _raw(c.data, c.chunk_off, c.merges)
        assert (rc, n_out, passes) == (mbpe.ERR_ARG, 0, 0), c.name
    t = mbpe.Tokenizer("")
    t.set_special_tokens_from_file(b"<|big|> 2147483646\n")
    t.set_merges(np.array([[97, 98]], dtype=np.uint32))
    assert t.encode(b"ab<|big|>ab").tolist() == [256, 2147483646, 256]
    with pytest.raises(mbpe.MbpeError) as e:
        t.encode(b"ab<|big|>ab", device=0)
    assert e.value.code == mbpe.ERR_ARG


def test_lookup_tables(dev):
    cases = E.lookup_cases()
    assert [len(c.merges) for c in cases] == [1, 7, 8, (1 << 15) - 1, 1 << 15, 100000, 50]
    for c in cases:
        _check(c, dev)
    # the precondition of the last case, on the Python mirror of pair_hash() and of the capacity rule and insertion loop
    # of encode_chunks() in csrc/encode.hip: at least four keys with a home in the last two slots lie behind the wrap
    slots, bits = E.build_table(cases[-1].merges.tolist())
    assert len(E.wrapped_keys(slots, bits)) >= 4 and E.tail_chain(slots, bits)[1] >= 6


def test_pass_counts_at_reduced_size(dev):
    """passes = 1 + the replacing passes of the deepest chunk: a property of the reference algorithm, so it is taken
    from the brute-force encode, on every case at 1/32 of the size."""
    for c in E.all_cases(SCALE):
        want, passes = brute_force_chunks(c)
        assert np.array_equal(O.encode_chunks(c.data, c.chunk_off, c.merges), want), c.name
        _check(c, dev, passes_want=passes)


# ---- the C-ABI's edges (include/mbpe.h) -----------------------------------------------------------------------------

def _raw(data, off, merges, cap=None, out=True, n_merges=None, merges_null=False, n_out=True, fn="mbpe_encode_chunks",
         n_chunks=None):
    text = np.ascontiguousarray(np.frombuffer(bytes(data), dtype=np.uint8) if isinstance(data, bytes) else data)
    off = None if off is None else np.ascontiguousarray(off, dtype=np.uint64)
    m = np.ascontiguousarray(merges, dtype=np.uint32).reshape(-1, 2)
    n, passes = ctypes.c_uint64(77), ctypes.c_uint32(77)
    cap = max(len(text), 1) if cap is None else cap
    buf = np.full((min(cap, len(text) + 8) if out else 0) + 2, 0xABABABAB, dtype=np.uint32)
    rc = getattr(mbpe.lib(), fn)(
        0, text.ctypes.data if len(text) else None, len(text), None if off is None else off.ctypes.data,
        (0 if off is None else len(off) - 1) if n_chunks is None else n_chunks,
        None if merges_null or not len(m) else m.ctypes.data, len(m) if n_merges is None else n_merges,
        buf.ctypes.data if out else None, cap, ctypes.byref(n) if n_out else None, ctypes.byref(passes))
    return rc, n.value, passes.value, buf


MERGES = np.array([[97, 98], [256, 99], [257, 257]], dtype=np.uint32)
TEXT = b"abcabcab" * 300 + b"c"


def test_capi_cap_and_size_query():
    want, deepest = brute_force_chunks(E.Case(np.frombuffer(TEXT, dtype=np.uint8), None, MERGES, "text"))
    assert np.array_equal(want, O.encode_chunks(TEXT, None, MERGES)) and deepest == 4
    rc, n, passes, buf = _raw(TEXT, None, MERGES, cap=len(want))
    assert (rc, n, passes) == (mbpe.OK, len(want), 4) and np.array_equal(buf[:n], want)
    assert (buf[n:] == 0xABABABAB).all()
    # cap one too small: MBPE_ERR_ARG, the count is reported, nothing is written
    rc, n, passes, buf = _raw(TEXT, None, MERGES, cap=len(want) - 1)
    assert (rc, n, passes) == (mbpe.ERR_ARG, len(want), 4) and (buf == 0xABABABAB).all()
    assert b"too small" in mbpe.lib().mbpe_last_error()
    # tokens_out NULL: a size query, whatever cap says
    for cap in (0, 5, 1 << 40):
        assert _raw(TEXT, None, MERGES, cap=cap, out=False)[:3] == (mbpe.OK, len(want), 4)
    # the same for the result left on the device
    assert _raw(TEXT, None, MERGES, cap=0, out=False, fn="mbpe_encode_chunks_device")[:3] == (mbpe.OK, len(want), 4)
    small = torch.zeros(len(want) - 1, dtype=torch.int32, device="cuda:0")
    with pytest.raises(mbpe.MbpeError) as e:
        mbpe.encode_chunks_device(TEXT, None, MERGES, small.data_ptr(), small.numel())
    assert e.value.code == mbpe.ERR_ARG and not small.any()
    # n_out is required
    assert _raw(TEXT, None, MERGES, n_out=False)[0] == mbpe.ERR_ARG


def test_capi_chunk_offsets():
    n = len(TEXT)
    for off in ([0, 9, 6, n], [0, 2 * n, n], [0, n + 64, n], [0, 1 << 62, n], [0, 6, 6, 5, n]):        # descending
        rc, n_out, passes, buf = _raw(TEXT, np.array(off, dtype=np.uint64), MERGES)
        assert (rc, n_out, passes) == (mbpe.ERR_ARG, 0, 0) and (buf == 0xABABABAB).all(), off
    for off in ([0, 6, n - 1], [0, 6, n + 1], [1, 6, n], [0]):                            # not from 0 to n_bytes
        rc, n_out, passes, buf = _raw(TEXT, np.array(off, dtype=np.uint64), MERGES)
        assert (rc, n_out, passes) == (mbpe.ERR_ARG, 0, 0) and (buf == 0xABABABAB).all(), off
    # runs of empty chunks change nothing
    off = [0, 0, 0, 3, 3, 3, 3, 1025, 1025, n, n, n]
    want = O.encode_chunks(TEXT, np.array([0, 3, 1025, n], dtype=np.uint64), MERGES)
    rc, n_out, _, buf = _raw(TEXT, np.array(off, dtype=np.uint64), MERGES)
    assert rc == mbpe.OK and np.array_equal(buf[:n_out], want)
    assert np.array_equal(O.encode_chunks(TEXT, np.array(off, dtype=np.uint64), MERGES), want)
    # chunk_off NULL: one chunk, n_chunks ignored
    assert _raw(TEXT, None, MERGES, n_chunks=5)[:2] == (mbpe.OK, len(O.encode_chunks(TEXT, None, MERGES)))
    # an empty text, with and without chunks
    assert _raw(b"", None, MERGES)[:3] == (mbpe.OK, 0, 0)
    assert _raw(b"", np.array([0, 0, 0], dtype=np.uint64), MERGES)[:3] == (mbpe.OK, 0, 0)


def test_capi_merges_null():
    # no merges: the bytes as they are, one pass
    rc, n, passes, buf = _raw(TEXT, None, np.zeros((0, 2), dtype=np.uint32), merges_null=True)
    assert (rc, n, passes) == (mbpe.OK, len(TEXT), 1) and buf[:n].tolist() == list(TEXT)
    # NULL with a count is refused
    assert _raw(TEXT, None, MERGES, merges_null=True)[:3] == (mbpe.ERR_ARG, 0, 0)


# ---- beyond 2^32 bytes ----------------------------------------------------------------------------------------------

BLOCK = (1 << 20) + 7
COPIES = 4097


def test_encode_beyond_4_gib(dev):
    """4,097 copies of a block of 2^20 + 7 bytes (alphabet 3 with runs, 300 merges), one chunk each: 4.0005 GiB, no
    chunk start after the first on a span edge.  Every index of the passes is meant to be 64-bit (k_enc_widen, the span
    offsets, o + popc); the expected output is the block's encoding, once by the oracle, tiled.  Compared on the device,
    ids and chunk-end flags together.  Wall time of the encode call on an MI355X: see profiles/HISTORY.md."""
    n = BLOCK * COPIES
    assert n > 1 << 32
    free, total = torch.cuda.mem_get_info()
    need = 13 * n + (12 << 30)                       # text + three token arrays, the output here, the comparison
    if free < need:
        pytest.skip("%.1f GiB of device memory free, the case needs %.1f" % (free / 2**30, need / 2**30))
    block, merges = E.deep_block(5, BLOCK)
    assert len(block) == BLOCK
    enc = O.encode_chunks(block, None, merges)
    length = len(enc)
    row = enc.copy()
    row[-1] |= np.uint32(END)
    data = np.tile(block, COPIES)
    off = np.arange(COPIES + 1, dtype=np.uint64) * np.uint64(BLOCK)
    out = torch.zeros(COPIES * length + 1, dtype=torch.int32, device=dev)
    t0 = time.perf_counter()
    n_out, passes = mbpe.encode_chunks_device(data, off, merges, out.data_ptr(), out.numel())
    wall = time.perf_counter() - t0
    print("encode of %d bytes in %d chunks: %d tokens, %d passes, %.2f s" % (n, COPIES, n_out, passes, wall))
    del data
    assert n_out == COPIES * length and int(out[-1]) == 0
    want = torch.from_numpy(row.view(np.int32)).to(dev)
    diff = out[:-1].view(COPIES, length) != want
    if bool(diff.any()):
        at = int(diff.view(-1).nonzero()[0])
        pytest.fail("first difference at token %d (copy %d, token %d of %d): got %#x, want %#x; %d passes" % (
            at, at // length, at % length, length, int(out[at]) & 0xFFFFFFFF, int(row[at % length]), passes))
    del diff, out, want
    torch.cuda.empty_cache()
