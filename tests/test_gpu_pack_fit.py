"""mbpe_pack_fit on the GPU against fit_cases.ref_fit, which builds every row from Python lists straight from the
rule in include/mbpe.h: ids, len, labels, pos, seg, doc_row and doc_col, exactly; and against the existing kernels
where the rule makes the layouts coincide."""
import ctypes
import itertools
import random

import numpy as np
import pytest
import torch

import mbpe
from fit_cases import NO_ROW, cu_of, grid_lengths, plan_outputs, ref_fit, ref_plan

pytestmark = pytest.mark.gpu

PAD, BOS, EOS = 9, 1, 2
GUARD = 64
_TOK = {16: np.uint16, 32: np.uint32}
_ID = {16: np.uint16, 32: np.uint32, 64: np.uint64}
_LAB = {16: np.uint16, 32: np.int32, 64: np.int64}
BOS_EOS = ((None, None), (BOS, None), (None, EOS), (BOS, EOS))
ALL = dict(labels=True, positions=True, segments=True, doc_row=True, doc_col=True)


@pytest.fixture(scope="module")
def dev():
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def flat(docs, bits=32):
    off = np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.uint64)
    tokens = np.array([t for d in docs for t in d], dtype=_TOK[bits])
    return tokens, off


def as_arrays(ref, seq_len, out_bits):
    """ref_fit's lists as the arrays the library writes."""
    n = len(ref["len"])
    m = lambda k, dt: np.array(ref[k], dtype=np.int64).astype(dt).reshape(n, seq_len)
    return {"ids": m("ids", _ID[out_bits]), "lengths": np.array(ref["len"], dtype=np.uint32),
            "labels": m("labels", _LAB[out_bits]), "positions": m("pos", np.uint32), "segments": m("seg", np.uint32),
            "doc_row": np.array(ref["doc_row"], dtype=np.uint64), "doc_col": np.array(ref["doc_col"], dtype=np.uint32)}


def same(got, want, what):
    for k, w in want.items():
        if k in got:
            g = got[k]
            assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, g.shape, w.dtype, w.shape)
            if not np.array_equal(g, w):
                at = np.argwhere(g != w)[0]
                raise AssertionError("%s: %s differs first at %s: got %s, want %s" % (what, k, at, g[tuple(at)], w[tuple(at)]))


def docs_of(lens, rng, top=60000):
    return [[rng.randrange(10, top) for _ in range(n)] for n in lens]


# ---- the exact grid ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seq_len", [1, 2, 3, 5, 8, 9, 16, 33])
def test_exact_grid(dev, seq_len):
    # 3, 5, 9 and 33 make the 8-cell groups straddle rows
    rng = random.Random(seq_len)
    for bos, eos in BOS_EOS:
        docs = docs_of(grid_lengths(seq_len, (bos is not None) + (eos is not None)), rng)
        tokens, off = flat(docs)
        ref = ref_fit(docs, seq_len, bos, eos, PAD, -100)
        want = as_arrays(ref, seq_len, 32)
        got = mbpe.pack_fit(tokens, off, seq_len, pad_id=PAD, bos_id=bos, eos_id=eos, cu_seqlens=True, **ALL)
        assert set(got) == set(want) | {"cu_seqlens", "max_seqlen"}, (seq_len, bos, eos)
        same(got, want, (seq_len, bos, eos))
        cu, longest = cu_of(ref, seq_len)
        assert got["cu_seqlens"].tolist() == cu and got["max_seqlen"] == longest


# ---- widths, host and device outputs -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("token_bits,out_bits,ignore", [(16, 16, 65535), (16, 32, -100), (16, 64, -100), (32, 32, -100),
                                                        (32, 64, -100)])
def test_width_combinations(dev, token_bits, out_bits, ignore):
    rng = random.Random(out_bits * 100 + token_bits)
    top = 65535 if token_bits == 16 or out_bits == 16 else (1 << 31) - 3
    bos, eos, pad = (65534, 65533, 65535) if out_bits == 16 else (top - 5, top - 6, top - 7)
    for seq_len in (3, 5, 9, 33):                                        # unaligned row starts for 16-bit ids
        lens = grid_lengths(seq_len, 2)
        docs = [[top - rng.randrange(4) for _ in range(n)] for n in lens]
        want = as_arrays(ref_fit(docs, seq_len, bos, eos, pad, ignore), seq_len, out_bits)
        tokens, off = flat(docs, token_bits)
        kw = dict(out_bits=out_bits, pad_id=pad, bos_id=bos, eos_id=eos, ignore_label=ignore)
        got = mbpe.pack_fit(tokens, off, seq_len, **kw, **ALL)
        same(got, want, (token_bits, out_bits, seq_len, "host"))
        assert got["ids"].max() == (65535 if out_bits == 16 else top)
        if out_bits != 16:
            assert (got["labels"] == -100).any() and (got["labels"] > 0).any()
        if token_bits == 32:
            # device tokens as the encoder leaves them: bit 31 flags a chunk end and is cleared on read
            flagged = tokens | np.where(np.arange(len(tokens)) % 3 == 0, np.uint32(1 << 31), np.uint32(0)).astype(np.uint32)
            d_tok = torch.from_numpy(flagged.view(np.int32).copy()).to(dev)
            n, n_docs = len(want["lengths"]), len(docs)
            tdt = {32: torch.int32, 64: torch.int64}[out_bits]
            d_ids, d_lab = (torch.full((n, seq_len), -1, dtype=tdt, device=dev) for _ in range(2))
            d_len = torch.full((n,), -1, dtype=torch.int32, device=dev)
            d_row = torch.full((n_docs,), -1, dtype=torch.int64, device=dev)
            d_col = torch.full((n_docs,), -1, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            rows = mbpe.pack_fit(None, off, seq_len, **kw, tokens_ptr=d_tok.data_ptr(), n_tokens=len(tokens), token_bits=32,
                                 out_ptr=d_ids.data_ptr(), len_ptr=d_len.data_ptr(), cap_rows=n,
                                 labels_ptr=d_lab.data_ptr(), doc_row_ptr=d_row.data_ptr(), doc_col_ptr=d_col.data_ptr())
            torch.cuda.synchronize()
            assert rows == n
            same({"ids": d_ids.cpu().numpy().view(_ID[out_bits]), "labels": d_lab.cpu().numpy(),
                  "lengths": d_len.cpu().numpy().view(np.uint32), "doc_row": d_row.cpu().numpy().view(np.uint64),
                  "doc_col": d_col.cpu().numpy().view(np.uint32)}, want, (token_bits, out_bits, seq_len, "device"))


def raw_fit(dev, tokens, off, spec, want, ignore=-100, cap_rows=None, n_rows=0):
    """mbpe_pack_fit into 16-byte aligned device buffers of exactly n_rows rows plus a guard, those of `want` (labels,
    pos, seg, doc_row, doc_col) only -> (code, n_rows, the buffers as host bytes; None where not asked, their sizes)."""
    cells, n_docs = n_rows * spec.seq_len, len(off) - 1
    sizes = [cells * spec.out_bits // 8, n_rows * 4, cells * spec.out_bits // 8, cells * 4, cells * 4, n_docs * 8, n_docs * 4]
    asked = [True, True] + [bool(w) for w in want]
    bufs = [torch.full((n + GUARD,), 0xAB, dtype=torch.uint8, device=dev) if a else None for n, a in zip(sizes, asked)]
    ptr = lambda b: None if b is None else b.data_ptr()
    assert all(b is None or b.data_ptr() % 16 == 0 for b in bufs)
    aux = mbpe.PackAux(ptr(bufs[2]), ptr(bufs[3]), ptr(bufs[4]), ignore)
    fit = mbpe.PackFit(ptr(bufs[5]), ptr(bufs[6]))
    got_rows = ctypes.c_uint64(77)
    torch.cuda.synchronize()
    rc = mbpe.lib().mbpe_pack_fit(0, tokens.ctypes.data if len(tokens) else None, len(tokens), tokens.dtype.itemsize * 8, 0,
                                  off.ctypes.data, n_docs, ctypes.byref(spec), ctypes.c_void_p(ptr(bufs[0])),
                                  n_rows if cap_rows is None else cap_rows, 1, ctypes.c_void_p(ptr(bufs[1])),
                                  ctypes.byref(got_rows), ctypes.byref(aux), ctypes.byref(fit))
    torch.cuda.synchronize()
    host = [None if b is None else b.cpu().numpy() for b in bufs]
    return rc, got_rows.value, host, sizes


NAMES = ["ids", "lengths", "labels", "positions", "segments", "doc_row", "doc_col"]


def test_device_outputs_in_every_combination(dev):
    rng = random.Random(31)
    seq_len = 5
    docs = docs_of([0, 4, 9, 1, 0, 23, 3, 8, 2], rng)
    tokens, off = flat(docs)
    spec = mbpe.pack_spec(seq_len, "packed", out_bits=64, pad_id=PAD, eos_id=EOS)
    ref = as_arrays(ref_fit(docs, seq_len, None, EOS, PAD, -100), seq_len, 64)
    n_rows = len(ref["lengths"])
    assert (n_rows * seq_len) % 8                                        # a partial last group
    for want in itertools.product((0, 1), repeat=5):
        rc, got_rows, host, sizes = raw_fit(dev, tokens, off, spec, want, n_rows=n_rows)
        assert (rc, got_rows) == (mbpe.OK, n_rows), want
        for name, h, n in zip(NAMES, host, sizes):
            if h is None:
                continue
            assert (h[n:] == 0xAB).all(), (want, name, "guard")
            assert np.array_equal(h[:n].view(ref[name].dtype).reshape(ref[name].shape), ref[name]), (want, name)


def test_cap_and_query(dev):
    rng = random.Random(32)
    docs = docs_of([7, 0, 30, 2], rng)
    tokens, off = flat(docs)
    spec = mbpe.pack_spec(6, "packed", pad_id=PAD, bos_id=BOS)
    n_rows = len(ref_fit(docs, 6, BOS, None, PAD, -100)["len"])
    n_out = ctypes.c_uint64(77)
    aux, fit = mbpe.PackAux(None, None, None, -100), mbpe.PackFit(None, None)
    rc = mbpe.lib().mbpe_pack_fit(0, tokens.ctypes.data, len(tokens), 32, 0, off.ctypes.data, len(off) - 1,
                                  ctypes.byref(spec), None, 0, 1, None, ctypes.byref(n_out), ctypes.byref(aux),
                                  ctypes.byref(fit))
    assert (rc, n_out.value) == (mbpe.OK, n_rows)
    # one row too few: nothing written, the count reported
    rc, got_rows, host, sizes = raw_fit(dev, tokens, off, spec, (1, 1, 1, 1, 1), cap_rows=n_rows - 1, n_rows=n_rows)
    assert (rc, got_rows) == (mbpe.ERR_ARG, n_rows) and b"too small" in mbpe.lib().mbpe_last_error()
    assert all((h == 0xAB).all() for h in host)
    rc, got_rows, host, sizes = raw_fit(dev, tokens, off, spec, (1, 1, 1, 1, 1), n_rows=n_rows)
    assert (rc, got_rows) == (mbpe.OK, n_rows)
    assert mbpe.pack_kernel_ms() > 0


def test_no_documents_and_documents_without_elements(dev):
    none = np.zeros(0, dtype=np.uint32)
    spec = mbpe.pack_spec(4, "packed", pad_id=PAD)
    rc, got_rows, host, sizes = raw_fit(dev, none, np.zeros(1, dtype=np.uint64), spec, (1, 1, 1, 1, 1))
    assert (rc, got_rows) == (mbpe.OK, 0) and all((h == 0xAB).all() for h in host)
    # five empty documents: no row, and doc_row says so, on the device too
    rc, got_rows, host, sizes = raw_fit(dev, none, np.zeros(6, dtype=np.uint64), spec, (1, 1, 1, 1, 1))
    assert (rc, got_rows) == (mbpe.OK, 0) and all((h == 0xAB).all() for h in host[:5])
    assert host[5][:40].view(np.uint64).tolist() == [NO_ROW] * 5 and (host[5][40:] == 0xAB).all()
    assert host[6][:20].view(np.uint32).tolist() == [0] * 5 and (host[6][20:] == 0xAB).all()
    got = mbpe.pack_fit(none, np.zeros(6, dtype=np.uint64), 4, **ALL)
    assert got["ids"].shape == (0, 4) and got["doc_row"].tolist() == [NO_ROW] * 5
    # with bos they are one element each and share rows of four
    got = mbpe.pack_fit(none, np.zeros(6, dtype=np.uint64), 4, pad_id=PAD, bos_id=BOS, **ALL)
    same(got, as_arrays(ref_fit([[]] * 5, 4, BOS, None, PAD, -100), 4, 32), "empty documents with bos")
    assert got["segments"].tolist() == [[1, 2, 3, 4], [5, 0, 0, 0]] and got["labels"][0].tolist() == [-100] * 4


# ---- many pieces per row, more groups than one pass of the grid ---------------------------------------------------------------

def test_many_documents(dev):
    # 20,000 documents of 0 .. 200 tokens in rows of 128: up to dozens of pieces in a row for the binary search.  Too
    # many cells for Python lists: the judge is the reference's placement, laid out with numpy
    S, n_docs = 128, 20000
    rng = np.random.default_rng(11)
    lens = rng.integers(0, 201, n_docs)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    tokens = (np.arange(int(off[-1])) % 60000 + 10).astype(np.uint16)
    placed, n_rows = ref_plan([int(n) + 1 for n in lens], S)              # with eos
    length, doc_row, doc_col = plan_outputs(placed, n_rows, n_docs)
    ids = np.full(n_rows * S, PAD, dtype=np.int64)
    lab = np.full(n_rows * S, -100, dtype=np.int64)
    pos, seg = np.zeros(n_rows * S, dtype=np.int64), np.zeros(n_rows * S, dtype=np.int64)
    tok64 = tokens.astype(np.int64)
    for row, col0, size, d, i in placed:
        E = np.concatenate([tok64[int(off[d]):int(off[d + 1])], [EOS]])
        k = np.arange(i * S, i * S + size)
        at = row * S + col0
        ids[at:at + size] = E[k]
        lab[at:at + size] = np.where(k + 1 < len(E), E[np.minimum(k + 1, len(E) - 1)], -100)
        pos[at:at + size], seg[at:at + size] = k, d + 1
    want = {"ids": ids.astype(np.uint32).reshape(n_rows, S), "labels": lab.astype(np.int32).reshape(n_rows, S),
            "positions": pos.astype(np.uint32).reshape(n_rows, S), "segments": seg.astype(np.uint32).reshape(n_rows, S),
            "lengths": np.array(length, dtype=np.uint32), "doc_row": np.array(doc_row, dtype=np.uint64),
            "doc_col": np.array(doc_col, dtype=np.uint32)}
    got = mbpe.pack_fit(tokens, off, S, pad_id=PAD, eos_id=EOS, **ALL)
    same(got, want, "20,000 documents")
    assert max(np.bincount([p[0] for p in placed])) >= 16                # pieces in the fullest row


# ---- where the rule makes the layouts coincide: the existing kernels, bit for bit --------------------------------------------

@pytest.mark.parametrize("out_bits", [16, 32, 64])
def test_identities_with_packed_and_padded(dev, out_bits):
    rng = random.Random(out_bits)
    ignore = 65535 if out_bits == 16 else -100
    for S, (bos, eos) in zip((3, 8, 9, 16), BOS_EOS):
        nbe = (bos is not None) + (eos is not None)
        kw = dict(out_bits=out_bits, pad_id=PAD, bos_id=bos, eos_id=eos, labels=True, positions=True, segments=True,
                  ignore_label=ignore)
        # every T_d a multiple of S (0 included, without bos and eos): the rows of PACKED
        docs = docs_of([rng.randrange(0 if nbe == 0 else 1, 4) * S - nbe for _ in range(23)], rng)
        tokens, off = flat(docs, 16)
        packed = mbpe.pack_tokens_aux(tokens, off, S, layout="packed", **kw)
        got = mbpe.pack_fit(tokens, off, S, **kw)
        for k in ("ids", "lengths", "labels", "positions", "segments"):
            assert got[k].dtype == packed[k].dtype and got[k].tobytes() == packed[k].tobytes(), ("packed", S, k)
        # every T_d one value in (S / 2, S]: no two share a row, the rows of PADDED
        for T in sorted({S // 2 + 1, S}):
            if T < nbe:
                continue
            docs = docs_of([T - nbe] * 23, rng)
            tokens, off = flat(docs, 16)
            padded = mbpe.pack_tokens_aux(tokens, off, S, layout="padded", **kw)
            got = mbpe.pack_fit(tokens, off, S, doc_row=True, doc_col=True, **kw)
            for k in ("ids", "lengths", "labels", "positions", "segments"):
                assert got[k].dtype == padded[k].dtype and got[k].tobytes() == padded[k].tobytes(), ("padded", S, T, k)
            assert got["doc_row"].tolist() == list(range(23)) and not got["doc_col"].any()
