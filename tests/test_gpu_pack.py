"""Id matrices on the GPU: mbpe_pack_tokens / mbpe_unpack_tokens, Encoder.encode_batch and the Tokenizer's
encode_batch_padded / decode_padded.

The judge is ref_pack below: the two layouts of include/mbpe.h restated with numpy as plain loops over the documents.
It shares no code with the library.  Every comparison is exact and on whole arrays.  Output buffers are prefilled with
0xAB bytes and are longer than the matrix: no expected id is 0xABAB.. (tokens stay below 40,000 or are 65,535), so
equality means every id was written, and the bytes around the matrix must keep their 0xAB.

The library works on streams of its own: whatever torch still has in flight on a buffer (its fill, its upload) is waited
for with torch.cuda.synchronize() before the buffer is handed over."""
import ctypes

import numpy as np
import pytest

import mbpe
import oracle as O
from conftest import read_data
from test_tokenizer_cpu import _golden_merges

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

PAD, BOS, EOS = 40001, 40002, 40003
GUARD = 256                                   # bytes behind every output
END = 0x80000000
DTYPES = {16: np.uint16, 32: np.uint32, 64: np.uint64}
COMBOS = [(16, 16), (16, 32), (16, 64), (32, 32), (32, 64)]         # (token_bits, out_bits): all that are allowed
SEQ_LENS = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 1023, 1024, 1025]


@pytest.fixture(scope="module")
def dev():
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


# ---- the layouts, restated ------------------------------------------------------------------------------------------

def ref_pack(tokens, off, seq_len, layout, out_bits, pad=PAD, bos=None, eos=None, pad_left=False, trunc_left=False):
    """-> (ids [n_rows, seq_len], lengths [n_rows]).  tokens: uint16, or uint32 whose bit 31 does not count."""
    ids = (np.asarray(tokens).astype(np.int64) & 0x7FFFFFFF).tolist()
    off = [int(o) for o in off]
    docs = [ids[off[i]:off[i + 1]] for i in range(len(off) - 1)]
    head = [] if bos is None else [bos]
    tail = [] if eos is None else [eos]
    rows, lengths = [], []
    if layout == "padded":
        keep = seq_len - len(head) - len(tail)
        for d in docs:
            body = d[:keep]
            if trunc_left:
                body = d[len(d) - keep:] if len(d) > keep else d
            row = head + body + tail
            fill = [pad] * (seq_len - len(row))
            rows.append(fill + row if pad_left else row + fill)
            lengths.append(len(row))
    else:
        stream = []
        for d in docs:
            stream += head + d + tail
        for at in range(0, len(stream), seq_len):
            row = stream[at:at + seq_len]
            lengths.append(len(row))
            rows.append(row + [pad] * (seq_len - len(row)))
    m = np.array(rows, dtype=DTYPES[out_bits]).reshape(len(rows), seq_len)
    return m, np.array(lengths, dtype=np.uint32)


def make_tokens(rng, lens, token_bits):
    """Random ids below 40,000 with some 65,535; 32-bit tokens carry bit 31 on the last token of every document."""
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    n = int(off[-1])
    t = rng.integers(0, 40000, size=n, dtype=np.uint32)
    if n:
        t[rng.integers(0, n, size=max(n // 50, 1))] = 65535
    if token_bits == 32:
        ends = off[1:][off[1:] > off[:-1]].astype(np.int64) - 1
        t[ends] |= END
    return t.astype(DTYPES[token_bits]), off


def doc_lens(rng, n_docs, seq_len, keep, turn):
    """Lengths up to 3 x seq_len, half of them 0, 1, keep - 1, keep, keep + 1; the first and the last document take
    those five in turn."""
    keep = max(keep, 0)                       # (PACKED takes a seq_len below nb + ne)
    special = [0, 1, max(keep - 1, 0), keep, keep + 1]
    lens = rng.integers(0, 3 * seq_len + 1, size=n_docs)
    pick = rng.random(n_docs) < 0.5
    lens[pick] = rng.choice(special, size=int(pick.sum()))
    if n_docs:
        lens[0] = special[turn % 5]
        lens[-1] = special[(turn // 5 + turn) % 5]
    return lens


# ---- the C function as it is ----------------------------------------------------------------------------------------

def raw_pack(dev, tokens, off, spec, tokens_on_device=False, shift=0, cap_rows=None, query=False):
    """mbpe_pack_tokens into prefilled device buffers that begin `shift` ids before the matrix and end GUARD bytes
    behind it -> (code, n_rows, ids [n_rows, seq_len] or None, lengths or None).  Asserts the guards."""
    L = mbpe.lib()
    t = np.ascontiguousarray(tokens)
    bits, ob = t.dtype.itemsize * 8, spec.out_bits // 8
    o = np.ascontiguousarray(off, dtype=np.uint64)
    n_rows = ctypes.c_uint64(77)
    keep = None
    tp = t.ctypes.data if len(t) else None
    if tokens_on_device and len(t):
        keep = torch.from_numpy(t.view(np.int16 if bits == 16 else np.int32).copy()).to(dev)
        tp = keep.data_ptr()
    head = (0, ctypes.c_void_p(tp) if tp else None, len(t), bits, int(bool(tokens_on_device and len(t))), o.ctypes.data,
            len(o) - 1, ctypes.byref(spec))
    assert L.mbpe_pack_tokens(*head, None, 0, 1, None, ctypes.byref(n_rows)) == mbpe.OK
    want_rows = n_rows.value
    if query:
        return mbpe.OK, want_rows, None, None
    n_id_bytes = want_rows * spec.seq_len * ob
    buf = torch.full((shift * ob + n_id_bytes + GUARD,), 0xAB, dtype=torch.uint8, device=dev)
    lbuf = torch.full((want_rows * 4 + GUARD,), 0xAB, dtype=torch.uint8, device=dev)
    n_rows.value = 77
    torch.cuda.synchronize()
    rc = L.mbpe_pack_tokens(*head, ctypes.c_void_p(buf.data_ptr() + shift * ob),
                            want_rows if cap_rows is None else cap_rows, 1, ctypes.c_void_p(lbuf.data_ptr()),
                            ctypes.byref(n_rows))
    torch.cuda.synchronize()
    raw, lraw = buf.cpu().numpy(), lbuf.cpu().numpy()
    if rc != mbpe.OK:
        assert (raw == 0xAB).all() and (lraw == 0xAB).all(), "a refused call wrote"
        return rc, n_rows.value, None, None
    assert n_rows.value == want_rows
    assert (raw[:shift * ob] == 0xAB).all(), "bytes in front of the matrix were written"
    assert (raw[shift * ob + n_id_bytes:] == 0xAB).all(), "bytes behind the matrix were written"
    assert (lraw[want_rows * 4:] == 0xAB).all(), "bytes behind the lengths were written"
    ids = raw[shift * ob:shift * ob + n_id_bytes].copy().view(DTYPES[spec.out_bits]).reshape(want_rows, spec.seq_len)
    return rc, want_rows, ids, lraw[:want_rows * 4].copy().view(np.uint32)


def check_pack(dev, tokens, off, seq_len, layout, out_bits, bos=None, eos=None, pad_left=False, trunc_left=False,
               tokens_on_device=False, shift=0, host_too=False, what=""):
    spec = mbpe.pack_spec(seq_len, layout, out_bits, PAD, bos, eos, pad_left, trunc_left)
    want, want_len = ref_pack(tokens, off, seq_len, layout, out_bits, PAD, bos, eos, pad_left, trunc_left)
    rc, n_rows, ids, lengths = raw_pack(dev, tokens, off, spec, tokens_on_device, shift)
    what = "%s seq_len %d %s %d->%d bos %s eos %s pad_left %d trunc_left %d dev %d shift %d" % (
        what, seq_len, layout, np.asarray(tokens).dtype.itemsize * 8, out_bits, bos, eos, pad_left, trunc_left,
        tokens_on_device, shift)
    assert rc == mbpe.OK and n_rows == len(want), what
    if not np.array_equal(ids, want):
        r, c = np.argwhere(ids != want)[0]
        pytest.fail("%s: ids[%d, %d] = %d, want %d" % (what, r, c, ids[r, c], want[r, c]))
    if not np.array_equal(lengths, want_len):
        r = int(np.flatnonzero(lengths != want_len)[0])
        pytest.fail("%s: len[%d] = %d, want %d" % (what, r, lengths[r], want_len[r]))
    if host_too:                                                  # the binding, host to host
        ids_h, len_h = mbpe.pack_tokens(tokens, off, seq_len, layout, out_bits, PAD, bos, eos, pad_left, trunc_left)
        assert ids_h.dtype == want.dtype and np.array_equal(ids_h, want) and np.array_equal(len_h, want_len), what
    return want, want_len


def _bos_eos(v, seq_len, layout):
    bos, eos = (BOS if v & 1 else None), (EOS if v & 2 else None)
    if layout == "padded" and seq_len < (bos is not None) + (eos is not None):
        eos = None
    return bos, eos


@pytest.mark.parametrize("seq_len", SEQ_LENS)
def test_padded_and_packed(dev, seq_len):
    """65 documents per call; over the calls of one seq_len every bit-width combination meets every pad_left /
    trunc_left setting, and bos / eos take their four settings in turn."""
    rng = np.random.default_rng(9000 + seq_len)
    i_seq = SEQ_LENS.index(seq_len)
    for i_c, (token_bits, out_bits) in enumerate(COMBOS):
        v = i_seq * len(COMBOS) + i_c
        for k, (layout, pad_left, trunc_left) in enumerate([("padded", 0, 0), ("padded", 1, 0), ("padded", 0, 1),
                                                            ("padded", 1, 1), ("packed", 0, 0)]):
            bos, eos = _bos_eos(v + k, seq_len, layout)
            keep = seq_len - (bos is not None) - (eos is not None)
            tokens, off = make_tokens(rng, doc_lens(rng, 65, seq_len, keep, v * 5 + k), token_bits)
            check_pack(dev, tokens, off, seq_len, layout, out_bits, bos, eos, pad_left, trunc_left,
                       tokens_on_device=(v + k) % 2 == 1, shift=(0, 1, 3)[(v + k) % 3], host_too=(k == i_c))


@pytest.mark.parametrize("n_docs", [0, 1, 2, 65, 4097])
def test_document_counts(dev, n_docs):
    rng = np.random.default_rng(9100 + n_docs)
    v = 0
    for seq_len in (1, 5, 16, 17):
        for layout in ("padded", "packed"):
            token_bits, out_bits = COMBOS[v % len(COMBOS)]
            bos, eos = _bos_eos(v, seq_len, layout)
            keep = seq_len - (bos is not None) - (eos is not None)
            tokens, off = make_tokens(rng, doc_lens(rng, n_docs, seq_len, keep, v), token_bits)
            pad_left, trunc_left = (v % 2, (v // 2) % 2) if layout == "padded" else (0, 0)
            check_pack(dev, tokens, off, seq_len, layout, out_bits, bos, eos, pad_left, trunc_left,
                       tokens_on_device=v % 2 == 0, shift=v % 4, what="%d docs" % n_docs)
            v += 1


def test_empty_documents_only(dev):
    empty16, empty32 = np.zeros(0, dtype=np.uint16), np.zeros(0, dtype=np.uint32)
    off = np.zeros(8, dtype=np.uint64)
    for layout in ("padded", "packed"):
        check_pack(dev, empty16, off, 3, layout, 16, what="empty")                       # PACKED: no row at all
        check_pack(dev, empty32, off, 3, layout, 64, bos=BOS, what="empty")              # rows of bos alone
        check_pack(dev, empty32, off, 4, layout, 32, bos=BOS, eos=EOS, what="empty")
    check_pack(dev, empty16, off, 4, "padded", 16, bos=BOS, eos=EOS, pad_left=True, trunc_left=True, what="empty")


def test_more_rows_than_a_grid_dimension(dev):
    """70,000 one-token documents at seq_len 2: more rows than 65,535."""
    rng = np.random.default_rng(9200)
    lens = np.ones(70000, dtype=np.int64)
    for token_bits, out_bits, layout, eos in ((16, 16, "padded", None), (32, 32, "padded", EOS), (16, 32, "packed", None),
                                              (32, 64, "packed", EOS)):
        tokens, off = make_tokens(rng, lens, token_bits)
        want, want_len = check_pack(dev, tokens, off, 2, layout, out_bits, eos=eos, tokens_on_device=True, what="70,000 docs")
        assert len(want) == (70000 if layout == "padded" or eos else 35000)


def test_sixteen_bit_documents_at_odd_offsets(dev):
    """Every document of the 16-bit input has an odd length, so every second one starts at an odd offset: no load may
    assume more than the token's own alignment.  Id 65,535 is a token like any other."""
    rng = np.random.default_rng(9300)
    lens = 2 * rng.integers(0, 20, size=200) + 1
    tokens, off = make_tokens(rng, lens, 16)
    tokens[::7] = 65535
    assert (off[1:-1:2] % 2 == 1).all() and (tokens == 65535).sum() > 100
    for seq_len in (7, 8, 16):
        for out_bits in (16, 32, 64):
            want, _ = check_pack(dev, tokens, off, seq_len, "padded", out_bits, trunc_left=True, tokens_on_device=True,
                                 what="odd offsets")
            assert (want == 65535).any()
            check_pack(dev, tokens, off, seq_len, "packed", out_bits, bos=BOS, tokens_on_device=True, what="odd offsets")
    # a token array that itself begins at an odd 16-bit offset of its allocation
    whole = torch.from_numpy(np.concatenate([[0], tokens]).astype(np.uint16).view(np.int16)).to(dev)
    spec = mbpe.pack_spec(8, "padded", 16, PAD)
    n_rows = ctypes.c_uint64()
    out = torch.full((len(lens) * 8 * 2 + GUARD,), 0xAB, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    assert mbpe.lib().mbpe_pack_tokens(0, ctypes.c_void_p(whole.data_ptr() + 2), len(tokens), 16, 1, off.ctypes.data,
                                       len(lens), ctypes.byref(spec), ctypes.c_void_p(out.data_ptr()), len(lens), 1, None,
                                       ctypes.byref(n_rows)) == mbpe.OK
    raw = out.cpu().numpy()
    want, _ = ref_pack(tokens, off, 8, "padded", 16)
    assert np.array_equal(raw[:len(lens) * 16].view(np.uint16).reshape(-1, 8), want) and (raw[len(lens) * 16:] == 0xAB).all()


def test_bit_31_of_32_bit_tokens_is_cleared(dev):
    rng = np.random.default_rng(9400)
    tokens, off = make_tokens(rng, rng.integers(1, 30, size=100), 32)
    assert ((tokens & END) != 0).sum() == 100
    for layout in ("padded", "packed"):
        for out_bits in (32, 64):
            want, _ = check_pack(dev, tokens, off, 9, layout, out_bits, tokens_on_device=True, what="flagged")
            assert (want < END).all()
            check_pack(dev, tokens & np.uint32(END - 1), off, 9, layout, out_bits, what="plain")


def test_query_and_cap(dev):
    rng = np.random.default_rng(9500)
    tokens, off = make_tokens(rng, rng.integers(0, 12, size=40), 16)
    for layout in ("padded", "packed"):
        spec = mbpe.pack_spec(5, layout, 16, PAD, BOS)
        want, _ = ref_pack(tokens, off, 5, layout, 16, PAD, BOS)
        assert raw_pack(dev, tokens, off, spec, query=True)[:2] == (mbpe.OK, len(want))
        for on_dev in (False, True):
            rc, n_rows, ids, _ = raw_pack(dev, tokens, off, spec, on_dev, cap_rows=len(want) - 1)   # asserts: nothing written
            assert (rc, n_rows, ids) == (mbpe.ERR_ARG, len(want), None)
            assert b"too small" in mbpe.lib().mbpe_last_error()
            rc, n_rows, ids, _ = raw_pack(dev, tokens, off, spec, on_dev, cap_rows=len(want) + 5)
            assert rc == mbpe.OK and np.array_equal(ids, want)
    # device output that is not aligned to its ids is refused
    spec = mbpe.pack_spec(5, "padded", 32, PAD)
    buf = torch.full((4096,), 0xAB, dtype=torch.uint8, device=dev)
    n_rows = ctypes.c_uint64()
    torch.cuda.synchronize()
    assert mbpe.lib().mbpe_pack_tokens(0, tokens.ctypes.data, len(tokens), 16, 0, off.ctypes.data, 40, ctypes.byref(spec),
                                       ctypes.c_void_p(buf.data_ptr() + 2), 40, 1, None, ctypes.byref(n_rows)) == mbpe.ERR_ARG
    assert n_rows.value == 40 and bool((buf == 0xAB).all())
    assert mbpe.pack_kernel_ms() > 0.0


def test_index_width(dev):
    """65,537 one-token documents at seq_len 65,536, 16 bits in and out: 2^32 + 65,536 ids, 8.6 GB, checked on the
    device.  An output index held in 32 bits would wrap in the last row."""
    n_docs, seq_len = 65537, 65536
    n_ids = n_docs * seq_len
    free = torch.cuda.mem_get_info(0)[0]
    if free < 20 * 1000 ** 3:
        pytest.skip("needs 20 GB of free device memory for the 8.6 GB matrix and its check, has %.1f GB" % (free / 1e9))
    rng = np.random.default_rng(9600)
    tokens = rng.integers(0, 40000, size=n_docs, dtype=np.uint16)
    tokens[-1] = 65535
    off = np.arange(n_docs + 1, dtype=np.uint64)
    d_tok = torch.from_numpy(tokens.view(np.int16)).to(dev)
    out = torch.full((n_ids * 2 + GUARD,), 0xAB, dtype=torch.uint8, device=dev)
    lengths = torch.full((n_docs * 4 + GUARD,), 0xAB, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    n_rows = mbpe.pack_tokens(None, off, seq_len, "padded", 16, PAD, tokens_ptr=d_tok.data_ptr(), n_tokens=n_docs,
                              token_bits=16, out_ptr=out.data_ptr(), len_ptr=lengths.data_ptr(), cap_rows=n_docs)
    torch.cuda.synchronize()
    assert n_rows == n_docs
    m = out[:n_ids * 2].view(torch.int16).view(n_docs, seq_len)
    assert torch.equal(m[:, 0], d_tok), "column 0 is not the tokens"
    pad16 = int(np.array(PAD, dtype=np.uint16).view(np.int16))
    assert int((m[:, 1:] != pad16).sum()) == 0, "an id beyond column 0 is not pad_id"
    assert bool((out[n_ids * 2:] == 0xAB).all()) and bool((lengths[n_docs * 4:] == 0xAB).all())
    assert bool((lengths[:n_docs * 4].view(torch.int32) == 1).all())


# ---- unpack -----------------------------------------------------------------------------------------------------------

def test_unpack_inverts_pack(dev):
    rng = np.random.default_rng(9700)
    merges = np.array([[97, 98], [256, 99], [257, 257]], dtype=np.uint32)
    for seq_len, token_bits, out_bits in ((1, 16, 16), (5, 16, 32), (16, 32, 32), (17, 32, 64), (1025, 16, 16)):
        lens = doc_lens(rng, 300 if seq_len < 100 else 20, seq_len, seq_len, seq_len)
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        tokens = rng.integers(0, 259, size=int(off[-1]), dtype=np.uint32).astype(DTYPES[token_bits])
        ids, lengths = mbpe.pack_tokens(tokens, off, seq_len, "padded", out_bits, PAD)
        docs = [tokens[int(a):int(b)][:seq_len] for a, b in zip(off[:-1], off[1:])]
        want = np.concatenate(docs).astype(np.uint32)
        want_off = np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.uint64)
        tb = np.uint16 if out_bits == 16 else np.uint32
        got, got_off = mbpe.unpack_tokens(ids, lengths, dtype=tb)                         # host to host
        assert got.dtype == tb and np.array_equal(got, want.astype(tb)) and np.array_equal(got_off, want_off), seq_len
        # device to device, with guards, then straight into the batch decode
        d_ids = torch.from_numpy(ids.view({16: np.int16, 32: np.int32, 64: np.int64}[out_bits])).to(dev)
        d_len = torch.from_numpy(lengths.view(np.int32)).to(dev)
        tsz = np.dtype(tb).itemsize
        d_out = torch.full((len(want) * tsz + GUARD,), 0xAB, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        n, dev_off = mbpe.unpack_tokens(None, None, dtype=tb, ids_ptr=d_ids.data_ptr(), len_ptr=d_len.data_ptr(),
                                        shape=ids.shape, id_bits=out_bits, out_ptr=d_out.data_ptr(), cap=len(want))
        raw = d_out.cpu().numpy()
        assert n == len(want) and np.array_equal(dev_off, want_off), seq_len
        assert np.array_equal(raw[:n * tsz].view(tb), want.astype(tb)) and (raw[n * tsz:] == 0xAB).all(), seq_len
        with mbpe.Decoder(merges) as dec:
            texts = dec.decode_batch([d.astype(np.uint32) for d in docs])
            back = torch.zeros(sum(len(t) for t in texts) + 1, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            byte_off, n_bytes, bad = dec.decode_batch_device(d_out.data_ptr(), n, dev_off, back.data_ptr(), back.numel(),
                                                             token_bits=tsz * 8)
            assert bad == 0 and back[:n_bytes].cpu().numpy().tobytes() == b"".join(texts), seq_len
        # a cap too small writes nothing; a length beyond seq_len is refused, also from device memory
        d_out.fill_(0xAB)
        torch.cuda.synchronize()
        with pytest.raises(mbpe.MbpeError) as e:
            mbpe.unpack_tokens(None, None, dtype=tb, ids_ptr=d_ids.data_ptr(), len_ptr=d_len.data_ptr(), shape=ids.shape,
                               id_bits=out_bits, out_ptr=d_out.data_ptr(), cap=len(want) - 1)
        assert e.value.code == mbpe.ERR_ARG and bool((d_out == 0xAB).all())
        d_len[len(lens) // 2] = seq_len + 1
        torch.cuda.synchronize()
        with pytest.raises(mbpe.MbpeError) as e:
            mbpe.unpack_tokens(None, None, dtype=tb, ids_ptr=d_ids.data_ptr(), len_ptr=d_len.data_ptr(), shape=ids.shape,
                               id_bits=out_bits, out_ptr=d_out.data_ptr(), cap=len(want) + seq_len)
        assert e.value.code == mbpe.ERR_ARG and bool((d_out == 0xAB).all())
        bad_len = lengths.copy()
        bad_len[0] = seq_len + 1
        with pytest.raises(mbpe.MbpeError) as e:
            mbpe.unpack_tokens(ids, bad_len)
        assert e.value.code == mbpe.ERR_ARG


# ---- Encoder.encode_batch -----------------------------------------------------------------------------------------------

MODELS = [("shakespeare_basic_lexical_512", "shakespeare.txt", 2500), ("taylorswift_basic_lexical_512", "taylorswift.txt", 900),
          ("taylorswift_gpt4_lexical_512", "taylorswift.txt", 700)]


@pytest.mark.parametrize("model,text,n_lines", MODELS)
def test_encoder_encode_batch(dev, model, text, n_lines):
    """Chunks are lines, documents runs of 0 to 3 lines: encode_batch == ref_pack(encode(..., offsets=True))."""
    rng = np.random.default_rng(9800)
    lines = read_data(text).splitlines(keepends=True)[:n_lines]
    assert len(lines) == n_lines and max(len(x) for x in lines) < sum(len(x) for x in lines) // 4      # pieces of a quarter
    data = np.frombuffer(b"".join(lines), dtype=np.uint8)
    chunk_off = np.concatenate([[0], np.cumsum([len(x) for x in lines])]).astype(np.uint64)
    cuts = [0]
    while cuts[-1] < len(lines):
        cuts.append(min(cuts[-1] + int(rng.integers(0, 4)), len(lines)))
    doc_chunk_off = np.array([0] + cuts + [len(lines)], dtype=np.uint64)      # an empty document first and last
    with mbpe.Encoder(_golden_merges(model)) as enc:
        tokens, tok_off = enc.encode(data, chunk_off, offsets=True)
        doc_tok_off = tok_off[doc_chunk_off.astype(np.int64)]
        d_text = torch.from_numpy(data.copy()).to(dev)
        torch.cuda.synchronize()
        settings = [dict(seq_len=17, layout="padded", out_bits=32, pad_id=PAD),
                    dict(seq_len=64, layout="packed", out_bits=64, pad_id=PAD, eos_id=EOS),
                    dict(seq_len=9, layout="padded", out_bits=16, pad_id=PAD, bos_id=BOS, pad_left=True, trunc_left=True),
                    dict(seq_len=2048, layout="packed", out_bits=16, pad_id=PAD, bos_id=BOS)]
        for i, kw in enumerate(settings):
            want, want_len = ref_pack(tokens, doc_tok_off, kw["seq_len"], kw["layout"], kw["out_bits"], PAD,
                                      kw.get("bos_id"), kw.get("eos_id"), kw.get("pad_left", False), kw.get("trunc_left", False))
            for text_dev in (False, True):
                src = dict(text_ptr=d_text.data_ptr(), n_bytes=len(data)) if text_dev else {}
                buf = None if text_dev else data
                ids, lengths = enc.encode_batch(buf, chunk_off, doc_chunk_off, **src, **kw)          # host output
                assert enc.n_tokens == len(tokens)
                assert ids.dtype == want.dtype and np.array_equal(ids, want) and np.array_equal(lengths, want_len), (i, text_dev)
                assert enc.kernel_ms() > enc.pack_ms() > 0.0
                ob = kw["out_bits"] // 8                                                                 # device output
                d_ids = torch.full((want.size * ob + GUARD,), 0xAB, dtype=torch.uint8, device=dev)
                d_len = torch.full((len(want) * 4 + GUARD,), 0xAB, dtype=torch.uint8, device=dev)
                torch.cuda.synchronize()
                n_rows = enc.encode_batch(buf, chunk_off, doc_chunk_off, **src, **kw, out_ptr=d_ids.data_ptr(),
                                          len_ptr=d_len.data_ptr(), cap_rows=len(want))
                raw, lraw = d_ids.cpu().numpy(), d_len.cpu().numpy()
                assert n_rows == len(want) and (raw[want.size * ob:] == 0xAB).all() and (lraw[len(want) * 4:] == 0xAB).all()
                assert np.array_equal(raw[:want.size * ob].view(want.dtype).reshape(want.shape), want), (i, text_dev)
                assert np.array_equal(lraw[:len(want) * 4].view(np.uint32), want_len), (i, text_dev)
        # a repeat call allocates nothing; the flat tokens stay where they are between the calls
        kw = settings[0]
        want, want_len = ref_pack(tokens, doc_tok_off, 17, "padded", 32)
        enc.encode_batch(data, chunk_off, doc_chunk_off, **kw)
        a = enc.alloc_count()
        ids, lengths = enc.encode_batch(data, chunk_off, doc_chunk_off, **kw)
        assert enc.alloc_count() == a and np.array_equal(ids, want)
        half = len(lines) // 2
        enc.encode_batch(data[:int(chunk_off[half])], chunk_off[:half + 1], None, **kw)              # a smaller batch
        assert enc.alloc_count() == a
        # three pieces or more give the same matrix
        enc.set_option("piece_bytes", len(data) // 4)
        for kw in settings[:2]:
            want, want_len = ref_pack(tokens, doc_tok_off, kw["seq_len"], kw["layout"], kw["out_bits"], PAD,
                                      kw.get("bos_id"), kw.get("eos_id"))
            ids, lengths = enc.encode_batch(data, chunk_off, doc_chunk_off, **kw)
            assert np.array_equal(ids, want) and np.array_equal(lengths, want_len)
            ids, lengths = enc.encode_batch(None, chunk_off, doc_chunk_off, text_ptr=d_text.data_ptr(), n_bytes=len(data), **kw)
            assert np.array_equal(ids, want) and np.array_equal(lengths, want_len)
        enc.set_option("piece_bytes", 0)
        # a list of texts: every text one chunk and one document
        some = [bytes(x) for x in lines[:50]] + [b""]
        ids, lengths = enc.encode_batch(some, seq_len=12, pad_id=PAD)
        flat = [enc.encode(x) for x in some]
        want, want_len = ref_pack(np.concatenate(flat), np.concatenate([[0], np.cumsum([len(f) for f in flat])]), 12, "padded", 32)
        assert np.array_equal(ids, want) and np.array_equal(lengths, want_len)
        # the cap rule, and what does not fit 16 bits
        n_docs = len(doc_chunk_off) - 1
        d_ids = torch.full((n_docs * 17 * 4,), 0xAB, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        with pytest.raises(mbpe.MbpeError) as e:
            enc.encode_batch(data, chunk_off, doc_chunk_off, seq_len=17, out_ptr=d_ids.data_ptr(), len_ptr=0,
                             cap_rows=n_docs - 1)
        assert e.value.code == mbpe.ERR_ARG and bool((d_ids == 0xAB).all())
        with pytest.raises(mbpe.MbpeError) as e:
            enc.encode_batch(data, chunk_off, doc_chunk_off, seq_len=17, out_bits=16, pad_id=65536)
        assert e.value.code == mbpe.ERR_VOCAB
        with pytest.raises(mbpe.MbpeError) as e:
            enc.encode_batch(data, chunk_off, doc_chunk_off[:-1] + np.uint64(1), seq_len=17)       # does not begin at 0
        assert e.value.code == mbpe.ERR_ARG
        assert np.array_equal(enc.encode(data, chunk_off), tokens)                                    # still works


# ---- Tokenizer ----------------------------------------------------------------------------------------------------------

def test_tokenizer_round_trip(dev):
    tok = mbpe.Tokenizer(O.GPT4_SPLIT_PATTERN)
    tok.set_special_tokens_from_file(read_data("special1.txt"))
    tok.set_merges(_golden_merges("taylorswift_gpt4_first_512"))
    lines = read_data("taylorswift.txt").splitlines(keepends=True)[:120]
    at = next(i for i, x in enumerate(lines) if len(x) > 30)
    lines[at] = lines[at][:10] + b"<|fim_prefix|>" + lines[at][10:]
    lines += [b"", read_data("specialtokensample.txt"), b"x"]
    encoded = [tok.encode(x) for x in lines]
    assert 100258 in encoded[at].tolist() and max(len(e) for e in encoded) > 40 > min(len(e) for e in encoded)
    for L in (1, 16, 40):
        ids, lengths = tok.encode_batch_padded(lines, seq_len=L, pad_id=PAD)
        assert ids.shape == (len(lines), L) and ids.dtype == np.uint32
        for i, e in enumerate(encoded):
            assert lengths[i] == min(len(e), L) and np.array_equal(ids[i, :lengths[i]], e[:L]), (L, i)
            assert (ids[i, lengths[i]:] == PAD).all(), (L, i)
        texts = tok.decode_padded(ids, lengths)
        assert texts == [tok.decode(e[:L]) for e in encoded], L
    # bos / eos given as special ids stand in the rows, and decode_padded writes their strings
    bos, eos = 100257, 100276
    ids, lengths = tok.encode_batch_padded(lines, seq_len=16, pad_id=PAD, bos_id=bos, eos_id=eos)
    for i, e in enumerate(encoded):
        assert lengths[i] == min(len(e), 14) + 2 and ids[i, 0] == bos and ids[i, lengths[i] - 1] == eos, i
        assert np.array_equal(ids[i, 1:lengths[i] - 1], e[:14]), i
    texts = tok.decode_padded(ids, lengths)
    assert texts == [b"<|endoftext|>" + tok.decode(e[:14]) + b"<|endofprompt|>" for e in encoded]
    # the matrix on the device, as 64-bit ids a torch index tensor takes; and the packed rows
    d_ids = torch.full((len(lines), 16), -1, dtype=torch.int64, device=dev)
    d_len = torch.full((len(lines),), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    n_rows = tok.encode_batch_padded(lines, seq_len=16, out_bits=64, pad_id=PAD, bos_id=bos, eos_id=eos,
                                     out_ptr=d_ids.data_ptr(), len_ptr=d_len.data_ptr(), cap_rows=len(lines))
    assert n_rows == len(lines) and np.array_equal(d_ids.cpu().numpy(), ids.astype(np.int64))
    assert np.array_equal(d_len.cpu().numpy(), lengths.astype(np.int32))
    flat = np.concatenate(encoded)
    off = np.concatenate([[0], np.cumsum([len(e) for e in encoded])])
    want, want_len = ref_pack(flat, off, 128, "packed", 32, PAD, None, eos)
    ids, lengths = tok.encode_batch_padded(lines, seq_len=128, layout="packed", pad_id=PAD, eos_id=eos)
    assert np.array_equal(ids, want) and np.array_equal(lengths, want_len)
    tok.close()
