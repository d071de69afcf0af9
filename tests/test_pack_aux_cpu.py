"""CPU tests of the training-batch calls (mbpe_pack_tokens_aux, mbpe_pack_cu_seqlens, mbpe_encoder_encode_batch_aux,
mbpe_tok_encode_batch_aux_device): the symbols exist and are listed, mbpe_pack_cu_seqlens -- host arithmetic alone --
gives the reference list, every argument error has its code before any device call and writes nothing, and the host
arithmetic of csrc/pack_host.h passes its stand-alone check (tests/pack_check.cpp), plain and under ASan + UBSan.

The judge of the lists is ref_cu_seqlens below: per document, in Python lists, every cell of the stream gets its
(row, segment) and a boundary is where that pair changes.  It shares no code with the library."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import mbpe
from conftest import ROOT

HERE = os.path.dirname(os.path.abspath(__file__))
NEW = ("mbpe_pack_tokens_aux", "mbpe_pack_cu_seqlens", "mbpe_encoder_encode_batch_aux")
NEW_TOK = ("mbpe_tok_encode_batch_aux_device",)


def _has_gpu():
    import torch
    return torch.cuda.is_available()


def test_exports_and_the_aux_struct_match_the_headers():
    L = mbpe.lib()
    header = open(os.path.join(ROOT, "include", "mbpe.h")).read()
    declared = set(re.findall(r"MBPE_API[^;]*?\b(mbpe_\w+)\s*\(", header))
    tok_header = open(os.path.join(ROOT, "include", "mbpe_tokenizer.h")).read()
    tok_declared = set(re.findall(r"MBPE_API[^;]*?\b(mbpe_tok_\w+)\s*\(", tok_header))
    for s in NEW:
        assert s in declared and s in mbpe.EXPORTS and hasattr(L, s) and getattr(L, s).argtypes, s
    for s in NEW_TOK:
        assert s in tok_declared and s in mbpe.TOK_EXPORTS and hasattr(L, s) and getattr(L, s).argtypes, s
    # the aux calls take the arguments of their counterparts, then aux (and the offsets)
    assert L.mbpe_pack_tokens_aux.argtypes[:-1] == L.mbpe_pack_tokens.argtypes
    assert L.mbpe_encoder_encode_batch_aux.argtypes[:-2] == L.mbpe_encoder_encode_batch.argtypes
    assert L.mbpe_tok_encode_batch_aux_device.argtypes[:-2] == L.mbpe_tok_encode_batch_packed_device.argtypes
    for name in ("pack_tokens_aux", "pack_cu_seqlens", "PackAux"):
        assert hasattr(mbpe, name), name
    assert hasattr(mbpe.Encoder, "encode_batch_aux") and hasattr(mbpe.Tokenizer, "encode_batch_aux")
    body = re.search(r"typedef struct \{([^}]*)\} mbpe_pack_aux;", header).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(\w+)\s*(\*?)\s*(\w+);", body)
    assert [(t, p) for t, p, _ in fields] == [("void", "*"), ("uint32_t", "*"), ("uint32_t", "*"), ("int64_t", "")]
    assert [n for _, _, n in fields] == [f for f, _ in mbpe.PackAux._fields_] == ["labels", "pos", "seg", "ignore_label"]
    assert [t for _, t in mbpe.PackAux._fields_] == [ctypes.c_void_p] * 3 + [ctypes.c_int64]
    assert ctypes.sizeof(mbpe.PackAux) == 32


# ---- cu_seqlens ---------------------------------------------------------------------------------------------------------

def ref_cu_seqlens(off, seq_len, bos, eos):
    """-> (boundaries, longest run) of the runs of equal (row, segment) over the stream's cells."""
    nbe = (bos is not None) + (eos is not None)
    seg = []
    for d in range(len(off) - 1):
        seg += [d + 1] * (int(off[d + 1]) - int(off[d]) + nbe)
    cu = [f for f in range(len(seg)) if f == 0 or seg[f] != seg[f - 1] or f // seq_len != (f - 1) // seq_len]
    cu.append(len(seg))
    if not seg:
        cu = [0]
    return cu, max([b - a for a, b in zip(cu[:-1], cu[1:])], default=0)


def _cu(off, spec, out=True, cap=None, guard=4):
    """mbpe_pack_cu_seqlens as it is -> (code, n_seqs, max_seqlen, the prefilled buffer)."""
    o = np.ascontiguousarray(off, dtype=np.uint64)
    buf = np.full(256, -7, dtype=np.int32)
    n_seqs, longest = ctypes.c_uint64(77), ctypes.c_uint32(77)
    rc = mbpe.lib().mbpe_pack_cu_seqlens(o.ctypes.data, len(o) - 1, ctypes.byref(spec), buf.ctypes.data if out else None,
                                         (len(buf) - guard - 1) if cap is None else cap, ctypes.byref(n_seqs),
                                         ctypes.byref(longest))
    return rc, n_seqs.value, longest.value, buf


def _doc_sets(seq_len):
    L = seq_len
    return [
        [],                                   # n_docs 0
        [0], [0, 0, 0],                       # empty documents only
        [1], [1, 1, 1],                       # of one token
        [L, L], [2 * L, 1, L - 1 if L > 1 else 1],      # ending exactly at a row end: a duplicate boundary
        [0, 3 * L + 1, 0, 2],                 # spanning three rows, empty documents around it
        [L + 1, 0, 0, L - 1, 1, 2 * L],
    ]


@pytest.mark.parametrize("seq_len", [1, 2, 3, 8, 9])
def test_cu_seqlens_equal_the_reference_list(seq_len):
    for lens in _doc_sets(seq_len):
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        for bos, eos in ((None, None), (5, None), (None, 6), (5, 6)):
            want, want_longest = ref_cu_seqlens(off, seq_len, bos, eos)
            what = (seq_len, lens, bos, eos)
            spec = mbpe.pack_spec(seq_len, "packed", 32, 0, bos, eos)
            rc, n_seqs, longest, buf = _cu(off, spec, out=False)                           # the query
            assert (rc, n_seqs, longest) == (mbpe.OK, len(want) - 1, want_longest), what
            assert (buf == -7).all()
            rc, n_seqs, longest, buf = _cu(off, spec, cap=len(want) - 1)                    # the exact cap
            assert (rc, n_seqs, longest) == (mbpe.OK, len(want) - 1, want_longest), what
            assert buf[:len(want)].tolist() == want and (buf[len(want):] == -7).all(), what
            assert longest <= seq_len
            if len(want) > 1:                                                               # a cap too small
                rc, n_seqs, longest, buf = _cu(off, spec, cap=len(want) - 2)
                assert (rc, n_seqs, longest) == (mbpe.ERR_ARG, len(want) - 1, want_longest), what
                assert (buf == -7).all() and b"too small" in mbpe.lib().mbpe_last_error()
            cu, longest = mbpe.pack_cu_seqlens(off, seq_len, bos, eos)                      # the binding
            assert cu.dtype == np.int32 and cu.tolist() == want and longest == want_longest, what
    # n_stream == 0 gives [0]
    cu, longest = mbpe.pack_cu_seqlens([0], seq_len)
    assert cu.tolist() == [0] and longest == 0


def test_cu_seqlens_argument_errors():
    L = mbpe.lib()
    off = np.array([0, 3, 3, 10], dtype=np.uint64)
    ok = mbpe.pack_spec(4, "packed")
    n_seqs, longest = ctypes.c_uint64(77), ctypes.c_uint32(77)
    buf = np.full(64, -7, dtype=np.int32)
    tail = (buf.ctypes.data, 63, ctypes.byref(n_seqs), ctypes.byref(longest))
    # PADDED has no cu_seqlens: its sequences are its rows
    for spec in (mbpe.pack_spec(4), mbpe.pack_spec(4, "padded", pad_left=True)):
        assert L.mbpe_pack_cu_seqlens(off.ctypes.data, 3, ctypes.byref(spec), *tail) == mbpe.ERR_ARG
        assert (n_seqs.value, longest.value) == (0, 0) and (buf == -7).all() and b"PACKED" in L.mbpe_last_error()
    # NULL arguments, a bad spec, bad offsets
    assert L.mbpe_pack_cu_seqlens(None, 3, ctypes.byref(ok), *tail) == mbpe.ERR_ARG
    assert L.mbpe_pack_cu_seqlens(off.ctypes.data, 3, None, *tail) == mbpe.ERR_ARG
    assert L.mbpe_pack_cu_seqlens(off.ctypes.data, 3, ctypes.byref(ok), buf.ctypes.data, 63, None,
                                  ctypes.byref(longest)) == mbpe.ERR_ARG
    assert L.mbpe_pack_cu_seqlens(off.ctypes.data, 3, ctypes.byref(ok), buf.ctypes.data, 63, ctypes.byref(n_seqs),
                                  None) == mbpe.ERR_ARG
    zero = mbpe.pack_spec(0, "packed")
    assert L.mbpe_pack_cu_seqlens(off.ctypes.data, 3, ctypes.byref(zero), *tail) == mbpe.ERR_ARG
    for bad in ([1, 3, 10], [0, 5, 3, 10]):
        b = np.array(bad, dtype=np.uint64)
        assert L.mbpe_pack_cu_seqlens(b.ctypes.data, len(b) - 1, ctypes.byref(ok), *tail) == mbpe.ERR_ARG
    # a stream of 2^31 elements or more does not fit int32 offsets: refused from a synthetic offset array, cu_out NULL
    wide = mbpe.pack_spec(1 << 30, "packed")                     # (few rows: the query walks them)
    for top, spec, want in (((1 << 31) - 1, wide, mbpe.OK), (1 << 31, wide, mbpe.ERR_ARG), (1 << 40, ok, mbpe.ERR_ARG),
                            ((1 << 31) - 1, mbpe.pack_spec(4, "packed", eos_id=1), mbpe.ERR_ARG)):
        big = np.array([0, top], dtype=np.uint64)
        n_seqs.value = 77
        rc = L.mbpe_pack_cu_seqlens(big.ctypes.data, 1, ctypes.byref(spec), None, 0, ctypes.byref(n_seqs),
                                    ctypes.byref(longest))
        assert rc == want, (top, rc)
        if want != mbpe.OK:
            assert n_seqs.value == 0 and b"2^31" in L.mbpe_last_error()
    assert (buf == -7).all()


# ---- mbpe_pack_tokens_aux: argument errors before the device -------------------------------------------------------------

T16 = np.arange(10, dtype=np.uint16)
T32 = np.arange(10, dtype=np.uint32)
OFF = [0, 3, 3, 10]
FILL = 0xAB


def _pack_aux(tokens, off, spec, ignore=-100, aux_null=False, want=(1, 1, 1), out=True, cap=64, on_device=0, shift=(0, 0, 0, 0)):
    """mbpe_pack_tokens_aux as it is, into prefilled host buffers (with on_device=1 the same buffers are named as
    device memory: such a call must be refused before anything is done with them) -> (code, n_rows, the buffers)."""
    t = np.ascontiguousarray(tokens)
    o = np.ascontiguousarray(off, dtype=np.uint64)
    bufs = [np.full(8192, FILL, dtype=np.uint8) for _ in range(5)]          # ids, len, labels, pos, seg
    base = [b.ctypes.data + (-b.ctypes.data) % 16 for b in bufs]           # 16-byte aligned
    ids, ln, lab, pos, seg = base
    aux = mbpe.PackAux((lab + shift[1]) if want[0] else None, (pos + shift[2]) if want[1] else None,
                       (seg + shift[3]) if want[2] else None, ignore)
    n_rows = ctypes.c_uint64(77)
    rc = mbpe.lib().mbpe_pack_tokens_aux(
        0, t.ctypes.data if len(t) else None, len(t), t.dtype.itemsize * 8, 0, o.ctypes.data, len(o) - 1,
        ctypes.byref(spec), (ids + shift[0]) if out else None, cap, on_device, ln if out else None, ctypes.byref(n_rows),
        None if aux_null else ctypes.byref(aux))
    return rc, n_rows.value, bufs


def _untouched(bufs):
    return all((b == FILL).all() for b in bufs)


def test_aux_argument_errors_come_before_the_device():
    s16, s32, s64 = (mbpe.pack_spec(4, "packed", out_bits=b) for b in (16, 32, 64))
    cases = [
        (dict(aux_null=True), s32, T32, mbpe.ERR_ARG),
        # ignore_label: 16 bits hold 0 .. 65,535, 32 bits -2^31 .. 2^32 - 1
        (dict(ignore=-100), s16, T16, mbpe.ERR_VOCAB),
        (dict(ignore=-1), s16, T16, mbpe.ERR_VOCAB),
        (dict(ignore=65536), s16, T16, mbpe.ERR_VOCAB),
        (dict(ignore=-(1 << 31) - 1), s32, T32, mbpe.ERR_ARG),
        (dict(ignore=1 << 32), s32, T32, mbpe.ERR_ARG),
        (dict(ignore=-(1 << 63)), s32, T32, mbpe.ERR_ARG),
        # the range holds whether labels are asked for or not
        (dict(ignore=65536, want=(0, 0, 0)), s16, T16, mbpe.ERR_VOCAB),
        # a device pointer that is not 16-byte aligned: ids, labels, pos, seg in turn
        (dict(on_device=1, shift=(8, 0, 0, 0)), s32, T32, mbpe.ERR_ARG),
        (dict(on_device=1, shift=(0, 4, 0, 0)), s32, T32, mbpe.ERR_ARG),
        (dict(on_device=1, shift=(0, 0, 8, 0)), s64, T32, mbpe.ERR_ARG),
        (dict(on_device=1, shift=(0, 0, 0, 2)), s16, T16, mbpe.ERR_ARG),
        # and the rules of mbpe_pack_tokens still hold
        ({}, mbpe.pack_spec(0), T32, mbpe.ERR_ARG),
        ({}, mbpe.pack_spec(4, out_bits=16), T32, mbpe.ERR_VOCAB),
        ({}, mbpe.pack_spec(4, "packed", pad_left=True), T32, mbpe.ERR_ARG),
    ]
    for kw, spec, tokens, want in cases:
        if spec.out_bits == 16:
            kw.setdefault("ignore", 65535)
        rc, n_rows, bufs = _pack_aux(tokens, OFF, spec, **kw)
        assert rc == want, (kw, list(bytes(spec)), rc)
        assert n_rows == 0 and _untouched(bufs), kw
        assert mbpe.lib().mbpe_last_error()
    rc, n_rows, bufs = _pack_aux(T32, [0, 5, 3, 10], s32)
    assert (rc, n_rows) == (mbpe.ERR_ARG, 0) and _untouched(bufs)
    # the edges of the ranges are accepted: the query answers without a device
    for spec, tokens, ignore in ((s16, T16, 0), (s16, T16, 65535), (s32, T32, -(1 << 31)), (s32, T32, (1 << 32) - 1),
                                 (s64, T32, -(1 << 63)), (s64, T32, (1 << 63) - 1), (s32, T32, -100)):
        rc, n_rows, bufs = _pack_aux(tokens, OFF, spec, ignore=ignore, out=False)
        assert (rc, n_rows) == (mbpe.OK, 3) and _untouched(bufs), ignore
        rc, n_rows, bufs = _pack_aux(tokens, OFF, spec, ignore=ignore, cap=2)              # too small: the count alone
        assert (rc, n_rows) == (mbpe.ERR_ARG, 3) and _untouched(bufs), ignore
        assert b"too small" in mbpe.lib().mbpe_last_error()
    # an aux with all three pointers NULL is valid; nothing to write is no device call
    rc, n_rows, bufs = _pack_aux(T32, OFF, s32, want=(0, 0, 0), out=False)
    assert (rc, n_rows) == (mbpe.OK, 3)
    rc, n_rows, bufs = _pack_aux(np.zeros(0, dtype=np.uint32), [0], s32)
    assert (rc, n_rows) == (mbpe.OK, 0) and _untouched(bufs)
    out = mbpe.pack_tokens_aux(np.zeros(0, dtype=np.uint32), [0], 4, "packed", out_bits=64, labels=True, positions=True,
                               segments=True, cu_seqlens=True)
    assert list(out) == ["ids", "lengths", "labels", "positions", "segments", "cu_seqlens", "max_seqlen"]
    assert out["ids"].shape == out["labels"].shape == out["positions"].shape == out["segments"].shape == (0, 4)
    assert (out["labels"].dtype, out["positions"].dtype, out["segments"].dtype) == (np.int64, np.uint32, np.uint32)
    assert out["cu_seqlens"].tolist() == [0] and out["max_seqlen"] == 0


def test_encoder_and_tokenizer_aux_entry_points_check_their_arguments():
    L = mbpe.lib()
    spec = mbpe.pack_spec(4)
    text = np.frombuffer(b"abab", dtype=np.uint8)
    docs = np.array([0, 1], dtype=np.uint64)
    ids = np.full(16, 0xABABABAB, dtype=np.uint32)
    ln = np.full(4, 0xABABABAB, dtype=np.uint32)
    lab = np.full(16, 0xABABABAB, dtype=np.uint32)
    tok_off = np.full(4, 0xABABABAB, dtype=np.uint64)
    aux = mbpe.PackAux(lab.ctypes.data, None, None, -100)
    n_rows, n_tok = ctypes.c_uint64(77), ctypes.c_uint64(77)
    assert L.mbpe_encoder_encode_batch_aux(None, text.ctypes.data, 4, 0, None, 0, docs.ctypes.data, 1, ctypes.byref(spec),
                                           ids.ctypes.data, 4, 0, ln.ctypes.data, ctypes.byref(n_rows), ctypes.byref(n_tok),
                                           ctypes.byref(aux), tok_off.ctypes.data) == mbpe.ERR_ARG
    assert (n_rows.value, n_tok.value) == (0, 0)
    tok = mbpe.Tokenizer("")
    tok.set_merges(np.array([[97, 98]], dtype=np.uint32))
    doc_off = np.array([0, 2, 4], dtype=np.uint64)
    head = (tok._h, text.ctypes.data, doc_off.ctypes.data, 2, 0)
    mid = (ids.ctypes.data, 4, 0, ln.ctypes.data)
    n_rows.value = 77
    assert L.mbpe_tok_encode_batch_aux_device(*head, 0, ctypes.byref(spec), *mid, ctypes.byref(n_rows), None, None,
                                              tok_off.ctypes.data) == mbpe.ERR_ARG                   # aux NULL
    assert n_rows.value == 0
    assert L.mbpe_tok_encode_batch_aux_device(*head, -1, ctypes.byref(spec), *mid, ctypes.byref(n_rows), None,
                                              ctypes.byref(aux), tok_off.ctypes.data) == mbpe.ERR_ARG
    assert L.mbpe_tok_encode_batch_aux_device(*head, 0, None, *mid, ctypes.byref(n_rows), None, ctypes.byref(aux),
                                              tok_off.ctypes.data) == mbpe.ERR_ARG
    for a in (ids, ln, lab, tok_off):
        assert (a == a.dtype.type(0xABABABAB)).all()
    tok.close()


@pytest.mark.skipif(_has_gpu(), reason="checks the no-device failure path")
def test_no_cpu_fallback():
    rc, n_rows, bufs = _pack_aux(T32, OFF, mbpe.pack_spec(4, "packed"))
    assert (rc, n_rows) == (mbpe.ERR_NO_DEVICE, 3) and _untouched(bufs)
    rc, n_rows, bufs = _pack_aux(T32, OFF, mbpe.pack_spec(4), want=(0, 0, 0))
    assert (rc, n_rows) == (mbpe.ERR_NO_DEVICE, 3) and _untouched(bufs)
    with pytest.raises(mbpe.MbpeError) as e:
        mbpe.pack_tokens_aux(T32, OFF, 4, labels=True)
    assert e.value.code == mbpe.ERR_NO_DEVICE
    tok = mbpe.Tokenizer("")
    tok.set_merges(np.array([[97, 98]], dtype=np.uint32))
    with pytest.raises(mbpe.MbpeError) as e:
        tok.encode_batch_aux([b"abab", b"", b"ab"], 4, segments=True)
    assert e.value.code == mbpe.ERR_NO_DEVICE
    tok.close()
    # cu_seqlens needs no device
    cu, longest = mbpe.pack_cu_seqlens(OFF, 4)
    assert cu.tolist() == [0, 3, 4, 8, 10] and longest == 4


# ---- the host arithmetic as a stand-alone program ------------------------------------------------------------------------

FLAGS = {
    "plain": ["-O2"],
    "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
}


@pytest.mark.parametrize("build", sorted(FLAGS))
def test_pack_host_arithmetic(build, tmp_path):
    exe = str(tmp_path / "pack_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Wextra", "-Werror"] + FLAGS[build] +
                          ["-I" + os.path.join(ROOT, "minbpe-cc_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                           os.path.join(HERE, "pack_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    # 9 seq_lens x 3 settings of nb + ne x (6 lists by hand + 8 random ones)
    assert r.stdout.strip().endswith("ok: %d lists, 0 failures" % (9 * 3 * 14))
