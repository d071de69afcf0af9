"""Training batches on the GPU: mbpe_pack_tokens_aux (k_pack_aux: ids, labels, positions, segments from one walk),
Encoder.encode_batch_aux and Tokenizer.encode_batch_aux, with mbpe_pack_cu_seqlens of their offsets.

The judge is ref_aux below: the definitions of include/mbpe.h restated per document in Python lists -- a document as it
appears in the matrix is the element list E = [bos] body [eos]; cell (d, k) holds E[k], its label is E[k + 1] or
ignore_label, its position k, its segment d + 1; pad cells hold pad_id, ignore_label, 0, 0.  It shares no code with the
library.  Every comparison is exact and on whole arrays.  Output buffers are prefilled with 0xAB bytes and are longer
than the matrix: no expected value is 0xABAB.. (tokens stay below 40,000 or are 65,535, ignore labels are chosen
accordingly), so equality means every cell was written, and the bytes behind the matrix must keep their 0xAB."""
import ctypes
import itertools

import numpy as np
import pytest

import mbpe
import oracle as O
from conftest import read_data
from test_gpu_pack import BOS, COMBOS, DTYPES, EOS, GUARD, PAD, doc_lens, make_tokens, raw_pack, ref_pack
from test_tokenizer_cpu import _golden_merges

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SEQ_LENS = [1, 2, 3, 7, 8, 9, 64, 1025]
SUBSETS = list(itertools.product((0, 1), repeat=3))                # (labels, pos, seg): all eight
IGNORE = {16: 65000, 32: -100, 64: -100}
LAYOUTS = [("padded", 0, 0), ("padded", 1, 0), ("padded", 0, 1), ("padded", 1, 1), ("packed", 0, 0)]


@pytest.fixture(scope="module")
def dev():
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


# ---- the definitions, restated ------------------------------------------------------------------------------------------

def ref_aux(tokens, off, seq_len, layout, out_bits, pad=PAD, bos=None, eos=None, pad_left=False, trunc_left=False,
            ignore=-100):
    """-> (ids, lengths, labels, pos, seg); ids and labels [n_rows, seq_len] of out_bits unsigned bits (ignore
    truncated), pos and seg uint32."""
    toks = (np.asarray(tokens).astype(np.int64) & 0x7FFFFFFF).tolist()
    off = [int(o) for o in off]
    head = [] if bos is None else [bos]
    tail = [] if eos is None else [eos]
    ign = ignore & ((1 << out_bits) - 1)
    pad_cell = (pad, ign, 0, 0)
    rows, lengths = [], []
    cells_of = lambda d, E: [(E[k], E[k + 1] if k + 1 < len(E) else ign, k, d + 1) for k in range(len(E))]
    if layout == "padded":
        keep = seq_len - len(head) - len(tail)
        for d in range(len(off) - 1):
            doc = toks[off[d]:off[d + 1]]
            body = doc[:keep]
            if trunc_left and len(doc) > keep:
                body = doc[len(doc) - keep:]
            cells = cells_of(d, head + body + tail)
            fill = [pad_cell] * (seq_len - len(cells))
            rows.append(fill + cells if pad_left else cells + fill)
            lengths.append(len(cells))
    else:
        stream = []
        for d in range(len(off) - 1):
            stream += cells_of(d, head + toks[off[d]:off[d + 1]] + tail)
        for at in range(0, len(stream), seq_len):
            row = stream[at:at + seq_len]
            lengths.append(len(row))
            rows.append(row + [pad_cell] * (seq_len - len(row)))
    m = np.array(rows, dtype=np.uint64).reshape(len(rows), seq_len, 4)
    wide = DTYPES[out_bits]
    return (m[:, :, 0].astype(wide), np.array(lengths, dtype=np.uint32), m[:, :, 1].astype(wide),
            m[:, :, 2].astype(np.uint32), m[:, :, 3].astype(np.uint32))


# ---- the C function as it is --------------------------------------------------------------------------------------------

def raw_aux(dev, tokens, off, spec, want=(1, 1, 1), ignore=-100, tokens_on_device=False, cap_rows=None, query=False):
    """mbpe_pack_tokens_aux into prefilled torch tensors that end GUARD bytes behind the matrix, read back once ->
    (code, n_rows, [ids, lengths, labels, pos, seg]; None for what was not asked for).  Asserts the guards."""
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
    none = mbpe.PackAux(None, None, None, ignore)
    assert L.mbpe_pack_tokens_aux(*head, None, 0, 1, None, ctypes.byref(n_rows), ctypes.byref(none)) == mbpe.OK
    want_rows = n_rows.value
    if query:
        return mbpe.OK, want_rows, None
    cells = want_rows * spec.seq_len
    sizes = [cells * ob, want_rows * 4, cells * ob if want[0] else None, cells * 4 if want[1] else None,
             cells * 4 if want[2] else None]
    bufs = [None if n is None else torch.full((n + GUARD,), 0xAB, dtype=torch.uint8, device=dev) for n in sizes]
    ptr = lambda b: None if b is None else b.data_ptr()
    aux = mbpe.PackAux(ptr(bufs[2]), ptr(bufs[3]), ptr(bufs[4]), ignore)
    n_rows.value = 77
    torch.cuda.synchronize()
    rc = L.mbpe_pack_tokens_aux(*head, ctypes.c_void_p(bufs[0].data_ptr()), want_rows if cap_rows is None else cap_rows, 1,
                                ctypes.c_void_p(bufs[1].data_ptr()), ctypes.byref(n_rows), ctypes.byref(aux))
    torch.cuda.synchronize()
    raws = [None if b is None else b.cpu().numpy() for b in bufs]
    if rc != mbpe.OK:
        assert all(r is None or (r == 0xAB).all() for r in raws), "a refused call wrote"
        return rc, n_rows.value, None
    assert n_rows.value == want_rows
    out = []
    wide = DTYPES[spec.out_bits]
    for r, n, dt in zip(raws, sizes, (wide, np.uint32, wide, np.uint32, np.uint32)):
        if r is None:
            out.append(None)
            continue
        assert (r[n:] == 0xAB).all(), "bytes behind an output were written"
        a = r[:n].copy().view(dt)
        out.append(a if len(out) == 1 else a.reshape(want_rows, spec.seq_len))      # (the lengths: one per row)
    return rc, want_rows, out


NAMES = ("ids", "len", "labels", "pos", "seg")


def check_aux(dev, tokens, off, seq_len, layout, out_bits, bos=None, eos=None, pad_left=False, trunc_left=False,
              want=(1, 1, 1), tokens_on_device=False, host_too=False, what=""):
    ignore = IGNORE[out_bits]
    spec = mbpe.pack_spec(seq_len, layout, out_bits, PAD, bos, eos, pad_left, trunc_left)
    ref = ref_aux(tokens, off, seq_len, layout, out_bits, PAD, bos, eos, pad_left, trunc_left, ignore)
    rc, n_rows, got = raw_aux(dev, tokens, off, spec, want, ignore, tokens_on_device)
    what = "%s seq_len %d %s %d->%d bos %s eos %s pad_left %d trunc_left %d want %s dev %d" % (
        what, seq_len, layout, np.asarray(tokens).dtype.itemsize * 8, out_bits, bos, eos, pad_left, trunc_left, want,
        tokens_on_device)
    assert rc == mbpe.OK and n_rows == len(ref[0]), what
    for name, g, w, asked in zip(NAMES, got, ref, (1, 1) + tuple(want)):
        assert (g is not None) == bool(asked), what
        if g is None:
            continue
        if not np.array_equal(g, w):
            at = tuple(np.argwhere(g != w)[0])
            pytest.fail("%s: %s%s = %d, want %d" % (what, name, list(at), g[at], w[at]))
    if host_too:                                                  # the binding, host to host
        out = mbpe.pack_tokens_aux(tokens, off, seq_len, layout, out_bits, PAD, bos, eos, pad_left, trunc_left,
                                   labels=want[0], positions=want[1], segments=want[2], ignore_label=ignore)
        assert list(out) == ["ids", "lengths"] + [n for n, w in zip(("labels", "positions", "segments"), want) if w], what
        assert np.array_equal(out["ids"], ref[0]) and np.array_equal(out["lengths"], ref[1]), what
        for name, w in zip(("labels", "positions", "segments"), ref[2:]):
            if name in out:
                assert out[name].shape == w.shape and np.array_equal(out[name].view(w.dtype), w), (what, name)
    return ref


def _bos_eos(v, seq_len, layout):
    bos, eos = (BOS if v & 1 else None), (EOS if v & 2 else None)
    if layout == "padded" and seq_len < (bos is not None) + (eos is not None):
        eos = None
    return bos, eos


def aux_doc_lens(rng, n_docs, seq_len, keep):
    """doc_lens of test_gpu_pack (0, 1, keep - 1, keep, keep + 1 and random lengths up to 3 x seq_len) with, in
    front, the lengths the walk turns on: multiples of seq_len and one of 3 x seq_len + 1."""
    lens = doc_lens(rng, n_docs, seq_len, keep, int(rng.integers(0, 25)))
    fixed = [seq_len, 0, 3 * seq_len + 1, 2 * seq_len, 1, max(keep, 0) + 1, max(keep - 1, 0), 0, 0, max(keep, 0)]
    m = min(len(fixed), max(len(lens) - 2, 0))
    lens[1:1 + m] = fixed[:m]
    return lens


def test_the_reference_agrees_with_ref_pack_and_the_issue():
    """ref_aux's ids are ref_pack's; and one case by hand: [bos] a b [eos] | [bos] [eos] | [bos] c [eos] at seq_len 4."""
    tokens, off = np.array([10, 11, 12], dtype=np.uint32), [0, 2, 2, 3]
    ids, ln, lab, pos, seg = ref_aux(tokens, off, 4, "packed", 32, PAD, BOS, EOS, ignore=-100)
    I = (1 << 32) - 100
    assert ids.tolist() == [[BOS, 10, 11, EOS], [BOS, EOS, BOS, 12], [EOS, PAD, PAD, PAD]] and ln.tolist() == [4, 4, 1]
    assert lab.tolist() == [[10, 11, EOS, I], [EOS, I, 12, EOS], [I, I, I, I]]
    assert pos.tolist() == [[0, 1, 2, 3], [0, 1, 0, 1], [2, 0, 0, 0]]
    assert seg.tolist() == [[1, 1, 1, 1], [2, 2, 3, 3], [3, 0, 0, 0]]
    ids, ln, lab, pos, seg = ref_aux(tokens, off, 3, "padded", 32, PAD, None, EOS, pad_left=True, ignore=-100)
    assert ids.tolist() == [[10, 11, EOS], [PAD, PAD, EOS], [PAD, 12, EOS]]
    assert lab.tolist() == [[11, EOS, I], [I, I, I], [I, EOS, I]]
    assert pos.tolist() == [[0, 1, 2], [0, 0, 0], [0, 0, 1]] and seg.tolist() == [[1, 1, 1], [0, 0, 2], [0, 3, 3]]
    rng = np.random.default_rng(9900)
    for layout, pad_left, trunc_left in LAYOUTS:
        t, o = make_tokens(rng, rng.integers(0, 20, size=30), 32)
        a = ref_aux(t, o, 7, layout, 64, PAD, BOS, EOS, pad_left, trunc_left)
        b = ref_pack(t, o, 7, layout, 64, PAD, BOS, EOS, pad_left, trunc_left)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("seq_len", SEQ_LENS)
def test_both_layouts_against_the_reference(dev, seq_len):
    """21 documents per call (an odd row count: with an odd seq_len the cells are no multiple of 8); over the calls of
    one seq_len every bit-width combination meets every layout setting, bos / eos take their four settings and the
    subsets of {labels, pos, seg} their eight in turn."""
    rng = np.random.default_rng(9910 + seq_len)
    i_seq = SEQ_LENS.index(seq_len)
    n, partial = i_seq * 3, 0
    for i_c, (token_bits, out_bits) in enumerate(COMBOS):
        for k, (layout, pad_left, trunc_left) in enumerate(LAYOUTS):
            bos, eos = _bos_eos(i_seq + i_c + k, seq_len, layout)
            keep = seq_len - (bos is not None) - (eos is not None)
            tokens, off = make_tokens(rng, aux_doc_lens(rng, 21, seq_len, keep), token_bits)
            ref = check_aux(dev, tokens, off, seq_len, layout, out_bits, bos, eos, pad_left, trunc_left,
                            want=SUBSETS[n % 8] if n % 3 else (1, 1, 1), tokens_on_device=n % 2 == 1, host_too=(k == i_c))
            partial += ref[0].size % 8 != 0
            n += 1
    assert partial or seq_len % 8 == 0


def test_every_subset_of_the_outputs(dev):
    rng = np.random.default_rng(9920)
    for layout, seq_len, out_bits in (("padded", 7, 16), ("packed", 7, 16), ("packed", 9, 64), ("padded", 3, 32)):
        tokens, off = make_tokens(rng, aux_doc_lens(rng, 13, seq_len, seq_len - 2), 16)
        for want in SUBSETS:
            ref = check_aux(dev, tokens, off, seq_len, layout, out_bits, BOS, EOS, want=want, tokens_on_device=True,
                            host_too=out_bits == 64, what="subset")
        assert ref[0].size % 8 != 0


def test_truncated_documents_end_in_eos_or_ignore(dev):
    """PADDED rows of documents cut by truncation: the last kept token's label is eos if eos is set, else ignore_label
    -- never the token that was cut off."""
    tokens = np.arange(100, 140, dtype=np.uint32)
    off = [0, 10, 40]
    for trunc_left in (0, 1):
        for pad_left in (0, 1):
            _, _, lab, pos, _ = check_aux(dev, tokens, off, 6, "padded", 32, None, EOS, pad_left, trunc_left, what="cut")
            assert (lab[:, 4] == EOS).all() and (lab[:, 5] == (1 << 32) - 100).all() and pos[:, 5].tolist() == [5, 5]
            ids, _, lab, _, _ = check_aux(dev, tokens, off, 6, "padded", 32, BOS, None, pad_left, trunc_left, what="cut")
            assert (lab[:, 5] == (1 << 32) - 100).all() and ids[:, 5].tolist() == ([109, 139] if trunc_left else [104, 114])


def test_ids_and_lengths_equal_those_of_mbpe_pack_tokens(dev):
    """The same arguments through k_pack_padded / k_pack_stream and through k_pack_aux, on device and on host outputs,
    with and without the other outputs."""
    rng = np.random.default_rng(9930)
    n = 0
    for seq_len in (1, 5, 8, 17, 1025):
        for layout, pad_left, trunc_left in LAYOUTS:
            token_bits, out_bits = COMBOS[n % len(COMBOS)]
            bos, eos = _bos_eos(n, seq_len, layout)
            keep = seq_len - (bos is not None) - (eos is not None)
            tokens, off = make_tokens(rng, aux_doc_lens(rng, 33, seq_len, keep), token_bits)
            spec = mbpe.pack_spec(seq_len, layout, out_bits, PAD, bos, eos, pad_left, trunc_left)
            rc, n_rows, ids, lengths = raw_pack(dev, tokens, off, spec, tokens_on_device=n % 2 == 0)
            assert rc == mbpe.OK
            for want in ((0, 0, 0), (1, 1, 1)):
                rc, n_rows2, got = raw_aux(dev, tokens, off, spec, want, IGNORE[out_bits], tokens_on_device=n % 2 == 1)
                assert rc == mbpe.OK and n_rows2 == n_rows, (seq_len, layout)
                assert np.array_equal(got[0], ids) and np.array_equal(got[1], lengths), (seq_len, layout, want)
            ids_h, len_h = mbpe.pack_tokens(tokens, off, seq_len, layout, out_bits, PAD, bos, eos, pad_left, trunc_left)
            out = mbpe.pack_tokens_aux(tokens, off, seq_len, layout, out_bits, PAD, bos, eos, pad_left, trunc_left,
                                       labels=n % 2 == 0, segments=True, ignore_label=IGNORE[out_bits])
            assert out["ids"].dtype == ids_h.dtype and np.array_equal(out["ids"], ids_h), (seq_len, layout)
            assert np.array_equal(out["lengths"], len_h) and np.array_equal(ids_h, ids), (seq_len, layout)
            n += 1
    assert mbpe.pack_kernel_ms() > 0.0


@pytest.mark.parametrize("n_docs", [0, 1, 65, 4097])
def test_document_counts(dev, n_docs):
    rng = np.random.default_rng(9940 + n_docs)
    v = 0
    for seq_len in (1, 5, 16):
        for layout in ("padded", "packed"):
            token_bits, out_bits = COMBOS[v % len(COMBOS)]
            bos, eos = _bos_eos(v, seq_len, layout)
            keep = seq_len - (bos is not None) - (eos is not None)
            lens = doc_lens(rng, n_docs, seq_len, keep, v) if n_docs > 100 else aux_doc_lens(rng, n_docs, seq_len, keep)
            tokens, off = make_tokens(rng, lens, token_bits)
            pad_left, trunc_left = (v % 2, (v // 2) % 2) if layout == "padded" else (0, 0)
            check_aux(dev, tokens, off, seq_len, layout, out_bits, bos, eos, pad_left, trunc_left,
                      tokens_on_device=v % 2 == 0, what="%d docs" % n_docs)
            v += 1


def test_empty_documents(dev):
    empty16, empty32 = np.zeros(0, dtype=np.uint16), np.zeros(0, dtype=np.uint32)
    off = np.zeros(8, dtype=np.uint64)
    for layout in ("padded", "packed"):                           # only empty documents
        ref = check_aux(dev, empty16, off, 3, layout, 16, what="empty")                 # PACKED: no row at all
        assert len(ref[0]) == (7 if layout == "padded" else 0) and not ref[4].any()
        check_aux(dev, empty32, off, 3, layout, 64, bos=BOS, what="empty")              # rows of bos alone
        ref = check_aux(dev, empty32, off, 4, layout, 32, bos=BOS, eos=EOS, what="empty")
        assert sorted(set(ref[4].ravel().tolist()) - {0}) == list(range(1, 8))
    # empty documents between full ones: their numbers are skipped in seg
    tokens = np.arange(1, 12, dtype=np.uint16)
    off = [0, 0, 4, 4, 4, 9, 11, 11]
    for layout in ("padded", "packed"):
        ref = check_aux(dev, tokens, off, 5, layout, 16, what="gaps", host_too=True)
        assert sorted(set(ref[4].ravel().tolist())) == [0, 2, 5, 6]
    ref = check_aux(dev, tokens, off, 4, "packed", 32, eos=EOS, what="gaps")
    assert sorted(set(ref[4].ravel().tolist())) == [0, 1, 2, 3, 4, 5, 6, 7]


def test_query_and_cap(dev):
    rng = np.random.default_rng(9950)
    tokens, off = make_tokens(rng, rng.integers(0, 12, size=40), 16)
    for layout in ("padded", "packed"):
        spec = mbpe.pack_spec(5, layout, 16, PAD, BOS)
        ref = ref_aux(tokens, off, 5, layout, 16, PAD, BOS, ignore=65000)
        assert raw_aux(dev, tokens, off, spec, ignore=65000, query=True)[:2] == (mbpe.OK, len(ref[0]))
        for on_dev in (False, True):
            rc, n_rows, got = raw_aux(dev, tokens, off, spec, (1, 1, 1), 65000, on_dev, cap_rows=len(ref[0]) - 1)
            assert (rc, n_rows, got) == (mbpe.ERR_ARG, len(ref[0]), None)                  # (asserts: nothing written)
            assert b"too small" in mbpe.lib().mbpe_last_error()
            rc, n_rows, got = raw_aux(dev, tokens, off, spec, (1, 1, 1), 65000, on_dev, cap_rows=len(ref[0]) + 5)
            assert rc == mbpe.OK and all(np.array_equal(g, w) for g, w in zip(got, ref))
    # the binding with device pointers: the row count, and cu_seqlens when asked
    spec_kw = dict(seq_len=5, layout="packed", out_bits=16, pad_id=PAD, bos_id=BOS)
    ref = ref_aux(tokens, off, 5, "packed", 16, PAD, BOS, ignore=65000)
    n_rows = len(ref[0])
    d_ids = torch.zeros((n_rows, 5), dtype=torch.int16, device=dev)
    d_lab = torch.zeros((n_rows, 5), dtype=torch.int16, device=dev)
    d_seg = torch.zeros((n_rows, 5), dtype=torch.int32, device=dev)
    d_len = torch.zeros(n_rows, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    got = mbpe.pack_tokens_aux(tokens, off, **spec_kw, out_ptr=d_ids.data_ptr(), len_ptr=d_len.data_ptr(), cap_rows=n_rows,
                               labels_ptr=d_lab.data_ptr(), seg_ptr=d_seg.data_ptr(), ignore_label=65000, cu_seqlens=True)
    assert got[0] == n_rows and np.array_equal(d_ids.cpu().numpy().view(np.uint16), ref[0])
    assert np.array_equal(d_lab.cpu().numpy().view(np.uint16), ref[2])
    assert np.array_equal(d_seg.cpu().numpy().view(np.uint32), ref[4])
    assert got[1].tolist() == run_boundaries(ref[4], ref[1]) and got[2] == max(np.diff(got[1]))
    # a device output that is not 16-byte aligned is refused
    with pytest.raises(mbpe.MbpeError) as e:
        mbpe.pack_tokens_aux(tokens, off, **spec_kw, out_ptr=d_ids.data_ptr(), len_ptr=d_len.data_ptr(), cap_rows=n_rows,
                             seg_ptr=d_seg.data_ptr() + 8, ignore_label=65000)
    assert e.value.code == mbpe.ERR_ARG


def run_boundaries(seg, lengths):
    """The starts of the maximal runs of equal (row, seg) among the stream's cells of a PACKED matrix, and its end."""
    n_rows, seq_len = seg.shape
    n_stream = int(np.asarray(lengths, dtype=np.int64).sum())
    rows = np.repeat(np.arange(n_rows), seq_len)[:n_stream]
    s = seg.reshape(-1)[:n_stream]
    assert (s != 0).all() and not seg.reshape(-1)[n_stream:].any()
    cut = [f for f in range(n_stream) if f == 0 or s[f] != s[f - 1] or rows[f] != rows[f - 1]]
    return cut + [n_stream] if n_stream else [0]


def test_index_width(dev):
    """65,537 one-token documents with bos at seq_len 65,536, 16-bit ids and pos alone: 2^32 + 65,536 cells, 8.6 GB of
    ids and 17.2 GB of positions, checked on the device.  A cell index held in 32 bits would wrap in the last row."""
    n_docs, seq_len = 65537, 65536
    cells = n_docs * seq_len
    rng = np.random.default_rng(9960)
    tokens = rng.integers(0, 40000, size=n_docs, dtype=np.uint16)
    off = np.arange(n_docs + 1, dtype=np.uint64)
    d_tok = torch.from_numpy(tokens.view(np.int16)).to(dev)
    out = torch.full((cells * 2 + GUARD,), 0xAB, dtype=torch.uint8, device=dev)
    pos = torch.full((cells * 4 + GUARD,), 0xAB, dtype=torch.uint8, device=dev)
    lengths = torch.full((n_docs * 4 + GUARD,), 0xAB, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    n_rows = mbpe.pack_tokens_aux(None, off, seq_len, "padded", 16, PAD, bos_id=BOS, tokens_ptr=d_tok.data_ptr(),
                                  n_tokens=n_docs, token_bits=16, out_ptr=out.data_ptr(), len_ptr=lengths.data_ptr(),
                                  cap_rows=n_docs, pos_ptr=pos.data_ptr(), ignore_label=0)
    torch.cuda.synchronize()
    assert n_rows == n_docs
    m = out[:cells * 2].view(torch.int16).view(n_docs, seq_len)
    p = pos[:cells * 4].view(torch.int32).view(n_docs, seq_len)
    bos16, pad16 = (int(np.array(x, dtype=np.uint16).view(np.int16)) for x in (BOS, PAD))
    assert bool((m[:, 0] == bos16).all()) and torch.equal(m[:, 1], d_tok), "columns 0 and 1 are not bos and the tokens"
    assert bool((p[:, 0] == 0).all()) and bool((p[:, 1] == 1).all())
    assert int(p.sum(dtype=torch.int64)) == n_docs, "a position beyond column 1 is not 0"
    for r in (0, 65535, 65536):
        assert bool((m[r, 2:] == pad16).all()) and bool((p[r, 2:] == 0).all()), r
    flat_m, flat_p = m.view(-1), p.view(-1)                       # the cells on both sides of cell index 2^32
    at = 1 << 32
    assert flat_m[at - 2:at + 3].tolist() == [pad16, pad16, bos16, int(d_tok[65536]), pad16]
    assert flat_p[at - 2:at + 3].tolist() == [0, 0, 0, 1, 0]
    assert bool((out[cells * 2:] == 0xAB).all()) and bool((pos[cells * 4:] == 0xAB).all())
    assert bool((lengths[n_docs * 4:] == 0xAB).all()) and bool((lengths[:n_docs * 4].view(torch.int32) == 2).all())


# ---- Encoder and Tokenizer ----------------------------------------------------------------------------------------------

def _same(out, ref, what):
    assert np.array_equal(out["ids"], ref[0]) and np.array_equal(out["lengths"], ref[1]), what
    for name, w in zip(("labels", "positions", "segments"), ref[2:]):
        assert out[name].shape == w.shape and np.array_equal(out[name].view(w.dtype), w), (what, name)


def test_encoder_encode_batch_aux(dev):
    lines = read_data("taylorswift.txt").splitlines(keepends=True)[:200]
    lines[3] = b""                                                # an empty document
    data = np.frombuffer(b"".join(lines), dtype=np.uint8)
    chunk_off = np.concatenate([[0], np.cumsum([len(x) for x in lines])]).astype(np.uint64)
    all_four = dict(labels=True, positions=True, segments=True)
    with mbpe.Encoder(_golden_merges("taylorswift_basic_lexical_512")) as enc:
        tokens, tok_off = enc.encode(data, chunk_off, offsets=True)
        settings = [dict(seq_len=24, layout="padded", out_bits=32, pad_id=PAD, eos_id=EOS, trunc_left=True),
                    dict(seq_len=64, layout="packed", out_bits=64, pad_id=PAD, bos_id=BOS, eos_id=EOS),
                    dict(seq_len=33, layout="packed", out_bits=16, pad_id=PAD)]
        for kw in settings:
            ignore = IGNORE[kw["out_bits"]]
            ref = ref_aux(tokens, tok_off, kw["seq_len"], kw["layout"], kw["out_bits"], PAD, kw.get("bos_id"),
                          kw.get("eos_id"), False, kw.get("trunc_left", False), ignore)
            ids, lengths = enc.encode_batch(list(lines), **kw)
            packed = kw["layout"] == "packed"
            out = enc.encode_batch_aux(list(lines), **kw, **all_four, cu_seqlens=packed, ignore_label=ignore)
            assert np.array_equal(out["ids"], ids) and np.array_equal(out["lengths"], lengths), kw
            _same(out, ref, kw)
            assert enc.n_tokens == len(tokens) and np.array_equal(enc.doc_tok_off, tok_off), kw
            assert enc.kernel_ms() > enc.pack_ms() > 0.0
            if packed:
                cu, longest = mbpe.pack_cu_seqlens(enc.doc_tok_off, kw["seq_len"], kw.get("bos_id"), kw.get("eos_id"))
                assert cu.tolist() == out["cu_seqlens"].tolist() == run_boundaries(out["segments"], out["lengths"]), kw
                assert longest == out["max_seqlen"] == int(np.diff(cu).max()) <= kw["seq_len"]
            # the same into device memory, from a text in device memory
            ob = kw["out_bits"] // 8
            tdt = {16: torch.int16, 32: torch.int32, 64: torch.int64}[kw["out_bits"]]
            d_text = torch.from_numpy(data.copy()).to(dev)
            d_ids, d_lab = (torch.full(ref[0].shape, -1, dtype=tdt, device=dev) for _ in range(2))
            d_pos, d_seg = (torch.full(ref[0].shape, -1, dtype=torch.int32, device=dev) for _ in range(2))
            d_len = torch.full((len(ref[0]),), -1, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            n_rows = enc.encode_batch_aux(None, chunk_off, None, text_ptr=d_text.data_ptr(), n_bytes=len(data), **kw,
                                          out_ptr=d_ids.data_ptr(), len_ptr=d_len.data_ptr(), cap_rows=len(ref[0]),
                                          labels_ptr=d_lab.data_ptr(), pos_ptr=d_pos.data_ptr(), seg_ptr=d_seg.data_ptr(),
                                          ignore_label=ignore)
            assert n_rows == len(ref[0]) and np.array_equal(enc.doc_tok_off, tok_off)
            for t, w in zip((d_ids, d_len, d_lab, d_pos, d_seg), ref):
                assert np.array_equal(t.cpu().numpy().view(w.dtype), w), kw
            if kw["out_bits"] == 64:
                assert int(d_lab.min()) == -100                   # ignore_label as an int64 tensor reads it
        # a repeat call of no larger size allocates nothing
        kw = settings[1]
        enc.encode_batch_aux(list(lines), **kw, **all_four)
        a = enc.alloc_count()
        out = enc.encode_batch_aux(list(lines), **kw, **all_four)
        assert enc.alloc_count() == a
        enc.encode_batch_aux(list(lines[:100]), **kw, **all_four)
        assert enc.alloc_count() == a
        # 16-bit labels take no negative ignore_label
        with pytest.raises(mbpe.MbpeError) as e:
            enc.encode_batch_aux(list(lines), **settings[2], labels=True)
        assert e.value.code == mbpe.ERR_VOCAB


def test_tokenizer_encode_batch_aux(dev):
    tok = mbpe.Tokenizer(O.GPT4_SPLIT_PATTERN)
    tok.set_merges(_golden_merges("taylorswift_gpt4_lexical_512"))
    lines = read_data("taylorswift.txt").splitlines(keepends=True)[:200]
    lines[7] = b""
    encoded = tok.encode_batch(lines)
    flat = np.concatenate(encoded)
    off = np.concatenate([[0], np.cumsum([len(e) for e in encoded])]).astype(np.uint64)
    for kw in (dict(seq_len=48, layout="packed", pad_id=PAD, eos_id=EOS),
               dict(seq_len=16, layout="padded", pad_id=PAD, bos_id=BOS, pad_left=True, out_bits=64)):
        packed = kw["layout"] == "packed"
        ref = ref_aux(flat, off, kw["seq_len"], kw["layout"], kw.get("out_bits", 32), PAD, kw.get("bos_id"),
                      kw.get("eos_id"), kw.get("pad_left", False), False, -100)
        ids, lengths = tok.encode_batch_padded(lines, **kw)
        out = tok.encode_batch_aux(lines, **kw, labels=True, positions=True, segments=True, cu_seqlens=packed)
        assert np.array_equal(out["ids"], ids) and np.array_equal(out["lengths"], lengths), kw
        _same(out, ref, kw)
        assert np.array_equal(tok.doc_tok_off, off), kw
        assert int(out["labels"].min()) == -100
        if packed:
            cu, longest = mbpe.pack_cu_seqlens(tok.doc_tok_off, kw["seq_len"], None, EOS)
            assert cu.tolist() == out["cu_seqlens"].tolist() == run_boundaries(out["segments"], out["lengths"])
            assert longest == out["max_seqlen"]
    tok.close()
