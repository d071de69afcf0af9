"""mbpe_pack_windows on the GPU against window_cases.ref_windows, which builds every row from Python lists straight
from the rule in include/mbpe.h: ids, len, labels, pos, seg, row_doc and row_tok0, exactly."""
import ctypes
import itertools
import random

import numpy as np
import pytest
import torch

import mbpe
from window_cases import grid_lengths, ref_windows

pytestmark = pytest.mark.gpu

PAD, BOS, EOS = 9, 1, 2
GUARD = 64
_TOK = {16: np.uint16, 32: np.uint32}
_ID = {16: np.uint16, 32: np.uint32, 64: np.uint64}
_LAB = {16: np.uint16, 32: np.int32, 64: np.int64}


@pytest.fixture(scope="module")
def dev():
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def flat(docs, bits=32):
    off = np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.uint64)
    tokens = np.array([t for d in docs for t in d], dtype=_TOK[bits])
    return tokens, off


def as_arrays(ref, seq_len, out_bits):
    """ref_windows' lists as the arrays the library writes."""
    n = len(ref["len"])
    m = lambda k, dt: np.array(ref[k], dtype=np.int64).astype(dt).reshape(n, seq_len)
    return {"ids": m("ids", _ID[out_bits]), "lengths": np.array(ref["len"], dtype=np.uint32),
            "labels": m("labels", _LAB[out_bits]), "positions": m("pos", np.uint32), "segments": m("seg", np.uint32),
            "row_doc": np.array(ref["row_doc"], dtype=np.uint32), "row_tok0": np.array(ref["row_tok0"], dtype=np.uint64)}


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


ALL = dict(labels=True, positions=True, segments=True, row_doc=True, row_tok0=True)


# ---- the exact grid ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seq_len", [3, 5, 8, 13, 16])
def test_exact_grid(dev, seq_len):
    rng = random.Random(seq_len)
    for bos, eos in ((None, None), (BOS, None), (None, EOS), (BOS, EOS)):
        keep = seq_len - (bos is not None) - (eos is not None)
        for stride in sorted({0, min(1, keep - 1), keep - 1}):
            step = keep - stride
            docs = docs_of(grid_lengths(keep, step), rng)
            tokens, off = flat(docs)
            for score_once in (0, 1):
                what = (seq_len, bos, eos, stride, score_once)
                want = as_arrays(ref_windows(docs, seq_len, stride, bos, eos, PAD, -100, score_once), seq_len, 32)
                got = mbpe.pack_windows(tokens, off, seq_len, stride, score_once=score_once, pad_id=PAD, bos_id=bos,
                                        eos_id=eos, **ALL)
                assert set(got) == set(want), what
                same(got, want, what)


# ---- widths --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("token_bits,out_bits,ignore", [(16, 16, 65535), (16, 32, -100), (16, 64, -100), (32, 32, -100),
                                                        (32, 64, -100)])
def test_width_combinations(dev, token_bits, out_bits, ignore):
    rng = random.Random(out_bits * 100 + token_bits)
    seq_len, stride = 8, 3
    top = 65535 if token_bits == 16 or out_bits == 16 else (1 << 31) - 3
    lens = [0, 1, 5, 6, 7, 11, 40, 0, 6, 300, 2]
    docs = [[top - rng.randrange(4) for _ in range(n)] for n in lens]
    bos, eos, pad = (65534, 65533, 65535) if out_bits == 16 else (top - 5, top - 6, top - 7)
    want = as_arrays(ref_windows(docs, seq_len, stride, bos, eos, pad, ignore, 1), seq_len, out_bits)
    tokens, off = flat(docs, token_bits)
    got = mbpe.pack_windows(tokens, off, seq_len, stride, score_once=True, out_bits=out_bits, pad_id=pad, bos_id=bos,
                            eos_id=eos, ignore_label=ignore, **ALL)
    same(got, want, (token_bits, out_bits, "host"))
    assert got["ids"].max() == (65535 if out_bits == 16 else top)
    if out_bits != 16:
        assert (got["labels"] == -100).any() and (got["labels"] > 0).any()
    if token_bits == 32:
        # device tokens as the encoder leaves them: bit 31 flags a chunk end and is cleared on read
        flagged = tokens | np.where(np.arange(len(tokens)) % 3 == 0, np.uint32(1 << 31), np.uint32(0)).astype(np.uint32)
        assert (flagged >> 31).any()
        d_tok = torch.from_numpy(flagged.view(np.int32).copy()).to(dev)
        n = len(want["lengths"])
        tdt = {32: torch.int32, 64: torch.int64}[out_bits]
        d_ids, d_lab = (torch.full((n, seq_len), -1, dtype=tdt, device=dev) for _ in range(2))
        d_len = torch.full((n,), -1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        rows = mbpe.pack_windows(None, off, seq_len, stride, score_once=True, out_bits=out_bits, pad_id=pad, bos_id=bos,
                                 eos_id=eos, ignore_label=ignore, tokens_ptr=d_tok.data_ptr(), n_tokens=len(tokens),
                                 token_bits=32, out_ptr=d_ids.data_ptr(), len_ptr=d_len.data_ptr(), cap_rows=n,
                                 labels_ptr=d_lab.data_ptr())
        torch.cuda.synchronize()
        assert rows == n
        same({"ids": d_ids.cpu().numpy().view(_ID[out_bits]), "labels": d_lab.cpu().numpy(),
              "lengths": d_len.cpu().numpy().view(np.uint32)}, want, (token_bits, out_bits, "device"))


# ---- more documents than one scan slice holds ----------------------------------------------------------------------------------

def test_scan_beyond_one_slice(dev):
    rng = random.Random(5000)
    docs = docs_of([rng.randrange(41) for _ in range(5000)], rng)        # five spans of 1,024 documents
    tokens, off = flat(docs, 16)
    want = as_arrays(ref_windows(docs, 8, 3, BOS, None, PAD, -100, 0), 8, 32)
    got = mbpe.pack_windows(tokens, off, 8, 3, pad_id=PAD, bos_id=BOS, **ALL)
    same(got, want, "5,000 documents")
    assert len(got["lengths"]) > 5000 and got["row_doc"][-1] == 4999


def test_scan_beyond_one_slice_of_spans(dev):
    # the scan runs over spans of 1,024 documents, 1,024 threads wide: beyond 2^20 documents a thread owns two spans.
    # Too many rows for Python lists, so the judge is numpy over the same rule: W_d, its prefix sum, a and len per row
    n_docs, seq_len, stride = (1 << 20) + 3000, 4, 1
    step = seq_len - stride
    rng = np.random.default_rng(7)
    lens = rng.integers(0, 3, n_docs)
    lens[rng.integers(0, n_docs, 2000)] = rng.integers(5, 40, 2000)      # long documents between the one-row ones
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    tokens = (np.arange(int(off[-1])) % 60000 + 10).astype(np.uint16)
    W = np.where(lens <= seq_len, 1, 1 + -((seq_len - lens) // step))
    row_doc = np.repeat(np.arange(n_docs), W)
    row_start = np.concatenate([[0], np.cumsum(W)])
    a = (np.arange(len(row_doc)) - row_start[row_doc]) * step
    got = mbpe.pack_windows(tokens, off, seq_len, stride, pad_id=PAD, row_doc=True, row_tok0=True)
    assert len(got["lengths"]) == row_start[-1] > n_docs
    assert np.array_equal(got["row_doc"], row_doc) and np.array_equal(got["row_tok0"], a)
    assert np.array_equal(got["lengths"], np.minimum(lens[row_doc] - a, seq_len))
    src = off[row_doc].astype(np.int64) + a                              # column c of a row holds tokens[src + c]
    for c in range(seq_len):
        inside = c < got["lengths"]
        assert np.array_equal(got["ids"][inside, c], tokens[src[inside] + c]) and (got["ids"][~inside, c] == PAD).all()


# ---- device outputs: every subset of the optional ones, guards behind each -----------------------------------------------------

def raw_windows(dev, tokens, off, spec, stride, score_once, want, ignore=-100, cap_rows=None, n_rows=0):
    """mbpe_pack_windows into 16-byte aligned device buffers of exactly n_rows rows plus a guard, those of `want`
    (labels, pos, seg, row_doc, row_tok0) only -> (code, n_rows, the buffers as host bytes; None where not asked)."""
    cells = n_rows * spec.seq_len
    sizes = [cells * spec.out_bits // 8, n_rows * 4, cells * spec.out_bits // 8, cells * 4, cells * 4, n_rows * 4, n_rows * 8]
    asked = [True, True] + [bool(w) for w in want]
    bufs = [torch.full((n + GUARD,), 0xAB, dtype=torch.uint8, device=dev) if a else None for n, a in zip(sizes, asked)]
    ptr = lambda b: None if b is None else b.data_ptr()
    assert all(b is None or b.data_ptr() % 16 == 0 for b in bufs)
    aux = mbpe.PackAux(ptr(bufs[2]), ptr(bufs[3]), ptr(bufs[4]), ignore)
    win = mbpe.PackWindow(stride, score_once, ptr(bufs[5]), ptr(bufs[6]))
    got_rows = ctypes.c_uint64(77)
    torch.cuda.synchronize()
    rc = mbpe.lib().mbpe_pack_windows(0, tokens.ctypes.data, len(tokens), tokens.dtype.itemsize * 8, 0, off.ctypes.data,
                                      len(off) - 1, ctypes.byref(spec), ctypes.c_void_p(ptr(bufs[0])),
                                      n_rows if cap_rows is None else cap_rows, 1, ctypes.c_void_p(ptr(bufs[1])),
                                      ctypes.byref(got_rows), ctypes.byref(aux), ctypes.byref(win))
    torch.cuda.synchronize()
    host = [None if b is None else b.cpu().numpy() for b in bufs]
    return rc, got_rows.value, host, sizes


def test_device_outputs_in_every_combination(dev):
    rng = random.Random(31)
    seq_len, stride = 5, 1                                               # cells no multiple of 8: a partial last group
    docs = docs_of([0, 4, 9, 1, 0, 23, 3, 8], rng)
    tokens, off = flat(docs)
    spec = mbpe.pack_spec(seq_len, out_bits=64, pad_id=PAD, eos_id=EOS)
    ref = as_arrays(ref_windows(docs, seq_len, stride, None, EOS, PAD, -100, 1), seq_len, 64)
    n_rows = len(ref["lengths"])
    assert (n_rows * seq_len) % 8
    names = ["ids", "lengths", "labels", "positions", "segments", "row_doc", "row_tok0"]
    for want in itertools.product((0, 1), repeat=5):
        rc, got_rows, host, sizes = raw_windows(dev, tokens, off, spec, stride, 1, want, n_rows=n_rows)
        assert (rc, got_rows) == (mbpe.OK, n_rows), want
        for name, h, n in zip(names, host, sizes):
            if h is None:
                continue
            assert (h[n:] == 0xAB).all(), (want, name, "guard")
            assert np.array_equal(h[:n].view(ref[name].dtype).reshape(ref[name].shape), ref[name]), (want, name)


def test_cap_and_query(dev):
    rng = random.Random(32)
    docs = docs_of([7, 0, 30, 2], rng)
    tokens, off = flat(docs)
    spec = mbpe.pack_spec(6, pad_id=PAD, bos_id=BOS)
    n_rows = len(ref_windows(docs, 6, 2, BOS, None, PAD, -100, 0)["len"])
    n_out = ctypes.c_uint64(77)
    aux, win = mbpe.PackAux(None, None, None, -100), mbpe.PackWindow(2, 0, None, None)
    rc = mbpe.lib().mbpe_pack_windows(0, tokens.ctypes.data, len(tokens), 32, 0, off.ctypes.data, len(off) - 1,
                                      ctypes.byref(spec), None, 0, 1, None, ctypes.byref(n_out), ctypes.byref(aux),
                                      ctypes.byref(win))
    assert (rc, n_out.value) == (mbpe.OK, n_rows)
    # one row too few: nothing written, the count reported
    rc, got_rows, host, sizes = raw_windows(dev, tokens, off, spec, 2, 0, (1, 1, 1, 1, 1), cap_rows=n_rows - 1, n_rows=n_rows)
    assert (rc, got_rows) == (mbpe.ERR_ARG, n_rows) and b"too small" in mbpe.lib().mbpe_last_error()
    assert all((h == 0xAB).all() for h in host)
    rc, got_rows, host, sizes = raw_windows(dev, tokens, off, spec, 2, 0, (1, 1, 1, 1, 1), n_rows=n_rows)
    assert (rc, got_rows) == (mbpe.OK, n_rows)
    assert mbpe.pack_kernel_ms() > 0


# ---- when every document fits, the rows are those of MBPE_PACK_PADDED ----------------------------------------------------------

@pytest.mark.parametrize("out_bits", [16, 32, 64])
def test_match_with_padded(dev, out_bits):
    rng = random.Random(out_bits)
    for seq_len, bos, eos in ((3, None, None), (8, BOS, EOS), (13, BOS, None), (16, None, EOS)):
        keep = seq_len - (bos is not None) - (eos is not None)
        docs = docs_of([rng.choice([0, 1, keep - 1, keep, rng.randrange(keep + 1)]) for _ in range(37)], rng)
        tokens, off = flat(docs, 16)
        ignore = 65535 if out_bits == 16 else -100
        kw = dict(out_bits=out_bits, pad_id=PAD, bos_id=bos, eos_id=eos, labels=True, positions=True, segments=True,
                  ignore_label=ignore)
        padded = mbpe.pack_tokens_aux(tokens, off, seq_len, layout="padded", **kw)
        for stride, score_once in ((0, False), (keep - 1, True)):
            got = mbpe.pack_windows(tokens, off, seq_len, stride, score_once=score_once, row_doc=True, row_tok0=True, **kw)
            for k in ("ids", "lengths", "labels", "positions", "segments"):
                assert got[k].dtype == padded[k].dtype and got[k].tobytes() == padded[k].tobytes(), (seq_len, stride, k)
            assert got["row_doc"].tolist() == list(range(37)) and not got["row_tok0"].any()
