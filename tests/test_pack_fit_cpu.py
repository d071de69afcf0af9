"""CPU tests of the fit layout (mbpe_pack_fit, mbpe_pack_fit_plan, mbpe_pack_fit_cu_seqlens,
mbpe_encoder_encode_batch_fit, mbpe_encoder_encode_batch_endmask_fit, mbpe_tok_encode_batch_fit_device): the symbols
exist, are listed and typed and the struct matches the header; every argument error has its code before any device call
and writes nothing; the planner and the one-shot query give the reference's rows without a device; cu_seqlens are the
run boundaries of the reference's segments; the planner of csrc/pack_fit.h passes its stand-alone check
(tests/pack_fit_check.cpp), plain and under ASan + UBSan; and the reference itself (fit_cases.ref_fit, which is the
specification) equals its naive twin and has the properties the rule promises."""
import ctypes
import os
import random
import re
import subprocess

import numpy as np
import pytest

import mbpe
from conftest import ROOT
from fit_cases import NO_ROW, cu_of, grid_lengths, plan_outputs, ref_fit, ref_fit_naive, ref_plan

HERE = os.path.dirname(os.path.abspath(__file__))
NEW = ("mbpe_pack_fit", "mbpe_pack_fit_plan", "mbpe_pack_fit_cu_seqlens", "mbpe_encoder_encode_batch_fit",
       "mbpe_encoder_encode_batch_endmask_fit")
NEW_TOK = ("mbpe_tok_encode_batch_fit_device",)
SEQ_LENS = [1, 2, 3, 5, 8, 13, 16, 64]
BOS_EOS = [(None, None), (5, None), (None, 6), (5, 6)]


def _has_gpu():
    import torch
    return torch.cuda.is_available()


def test_exports_and_the_fit_struct_match_the_headers():
    L = mbpe.lib()
    header = open(os.path.join(ROOT, "include", "mbpe.h")).read()
    declared = set(re.findall(r"MBPE_API[^;]*?\b(mbpe_\w+)\s*\(", header))
    tok_header = open(os.path.join(ROOT, "include", "mbpe_tokenizer.h")).read()
    tok_declared = set(re.findall(r"MBPE_API[^;]*?\b(mbpe_tok_\w+)\s*\(", tok_header))
    for s in NEW:
        assert s in declared and s in mbpe.EXPORTS and hasattr(L, s) and getattr(L, s).argtypes, s
    for s in NEW_TOK:
        assert s in tok_declared and s in mbpe.TOK_EXPORTS and hasattr(L, s) and getattr(L, s).argtypes, s
    # the fit calls take the arguments of their counterparts, then fit
    assert L.mbpe_pack_fit.argtypes[:-1] == L.mbpe_pack_tokens_aux.argtypes
    assert L.mbpe_encoder_encode_batch_fit.argtypes[:-1] == L.mbpe_encoder_encode_batch_aux.argtypes
    assert L.mbpe_encoder_encode_batch_endmask_fit.argtypes[:-1] == L.mbpe_encoder_encode_batch_endmask.argtypes
    assert L.mbpe_tok_encode_batch_fit_device.argtypes[:-1] == L.mbpe_tok_encode_batch_aux_device.argtypes
    assert L.mbpe_pack_fit_cu_seqlens.argtypes == L.mbpe_pack_cu_seqlens.argtypes
    assert len(L.mbpe_pack_fit_plan.argtypes) == 8
    for name in ("pack_fit", "pack_fit_plan", "pack_fit_cu_seqlens", "PackFit"):
        assert hasattr(mbpe, name), name
    assert hasattr(mbpe.Encoder, "encode_batch_fit") and hasattr(mbpe.Encoder, "encode_batch_endmask_fit")
    assert hasattr(mbpe.Tokenizer, "encode_batch_fit")
    body = re.search(r"struct mbpe_pack_fit \{([^}]*)\};", header).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(\w+)\s*(\*?)\s*(\w+);", body)
    assert [(t, p) for t, p, _ in fields] == [("uint64_t", "*"), ("uint32_t", "*")]
    assert [n for _, _, n in fields] == [f for f, _ in mbpe.PackFit._fields_] == ["doc_row", "doc_col"]
    assert [t for _, t in mbpe.PackFit._fields_] == [ctypes.c_void_p] * 2
    assert ctypes.sizeof(mbpe.PackFit) == 16 and mbpe.PackFit.doc_col.offset == 8
    # no new layout constant, and the existing structs are as they were
    assert set(re.findall(r"#define (MBPE_PACK_\w+)", header)) == {"MBPE_PACK_PADDED", "MBPE_PACK_PACKED"}
    assert ctypes.sizeof(mbpe.PackSpec) == 32 and ctypes.sizeof(mbpe.PackAux) == 32 and ctypes.sizeof(mbpe.PackWindow) == 24


# ---- argument errors before the device ------------------------------------------------------------------------------------

T16 = np.arange(10, dtype=np.uint16)
T32 = np.arange(10, dtype=np.uint32)
OFF = [0, 3, 3, 10]
FILL = 0xAB


def _fit(tokens, off, spec, ignore=-100, aux_null=False, fit_null=False, want=(1, 1, 1, 1, 1), out=True, cap=64,
         on_device=0, shift=(0, 0, 0, 0, 0, 0), n_docs=None):
    """mbpe_pack_fit as it is, into prefilled host buffers (with on_device=1 the same buffers are named as device
    memory: such a call must be refused before anything is done with them) -> (code, n_rows, the buffers)."""
    t = np.ascontiguousarray(tokens)
    o = np.ascontiguousarray(off, dtype=np.uint64)
    bufs = [np.full(8192, FILL, dtype=np.uint8) for _ in range(7)]          # ids, len, labels, pos, seg, doc_row, doc_col
    base = [b.ctypes.data + (-b.ctypes.data) % 16 for b in bufs]           # 16-byte aligned
    ids, ln, lab, pos, seg, drow, dcol = base
    aux = mbpe.PackAux((lab + shift[1]) if want[0] else None, (pos + shift[2]) if want[1] else None,
                       (seg + shift[3]) if want[2] else None, ignore)
    fit = mbpe.PackFit((drow + shift[4]) if want[3] else None, (dcol + shift[5]) if want[4] else None)
    n_rows = ctypes.c_uint64(77)
    rc = mbpe.lib().mbpe_pack_fit(
        0, t.ctypes.data if len(t) else None, len(t), t.dtype.itemsize * 8, 0, o.ctypes.data,
        len(o) - 1 if n_docs is None else n_docs, ctypes.byref(spec), (ids + shift[0]) if out else None, cap, on_device,
        ln if out else None, ctypes.byref(n_rows), None if aux_null else ctypes.byref(aux),
        None if fit_null else ctypes.byref(fit))
    return rc, n_rows.value, bufs


def _untouched(bufs):
    return all((b == FILL).all() for b in bufs)


def _spec(seq_len, **kw):
    return mbpe.pack_spec(seq_len, "packed", **kw)


def test_fit_argument_errors_come_before_the_device():
    s16, s32, s64 = (_spec(4, out_bits=b) for b in (16, 32, 64))
    packed = mbpe.PACK_PACKED
    cases = [
        (dict(aux_null=True), s32, T32, mbpe.ERR_ARG),
        (dict(fit_null=True), s32, T32, mbpe.ERR_ARG),
        # the layout: PACKED, and what PACKED refuses
        ({}, mbpe.pack_spec(4), T32, mbpe.ERR_ARG),
        ({}, mbpe.PackSpec(packed, 4, 32, 0, mbpe.NO_TOKEN, mbpe.NO_TOKEN, 1, 0), T32, mbpe.ERR_ARG),
        ({}, mbpe.PackSpec(packed, 4, 32, 0, mbpe.NO_TOKEN, mbpe.NO_TOKEN, 0, 1), T32, mbpe.ERR_ARG),
        ({}, mbpe.PackSpec(2, 4, 32, 0, mbpe.NO_TOKEN, mbpe.NO_TOKEN, 0, 0), T32, mbpe.ERR_ARG),
        ({}, _spec(0), T32, mbpe.ERR_ARG),
        # seg holds the document number + 1 in 32 bits (the count is checked before the offsets are read)
        (dict(n_docs=0xFFFFFFFF), s32, T32, mbpe.ERR_ARG),
        # the rules of mbpe_pack_tokens_aux: ignore_label, alignment of device outputs
        (dict(ignore=-100), s16, T16, mbpe.ERR_VOCAB),
        (dict(ignore=65536), s16, T16, mbpe.ERR_VOCAB),
        (dict(ignore=1 << 32), s32, T32, mbpe.ERR_ARG),
        (dict(on_device=1, shift=(8, 0, 0, 0, 0, 0)), s32, T32, mbpe.ERR_ARG),
        (dict(on_device=1, shift=(0, 4, 0, 0, 0, 0)), s32, T32, mbpe.ERR_ARG),
        (dict(on_device=1, shift=(0, 0, 8, 0, 0, 0)), s64, T32, mbpe.ERR_ARG),
        (dict(on_device=1, shift=(0, 0, 0, 2, 0, 0)), s16, T16, mbpe.ERR_ARG),
        (dict(on_device=1, shift=(0, 0, 0, 0, 4, 0)), s32, T32, mbpe.ERR_ARG),
        (dict(on_device=1, shift=(0, 0, 0, 0, 0, 2)), s32, T32, mbpe.ERR_ARG),
        # the MBPE_ERR_VOCAB rules of pack_check_spec
        ({}, s16, T32, mbpe.ERR_VOCAB),
        ({}, _spec(4, out_bits=16, pad_id=65536), T16, mbpe.ERR_VOCAB),
        ({}, _spec(4, out_bits=16, bos_id=70000), T16, mbpe.ERR_VOCAB),
        ({}, _spec(4, out_bits=8), T32, mbpe.ERR_ARG),
    ]
    for kw, spec, tokens, want in cases:
        if spec.out_bits == 16:
            kw.setdefault("ignore", 65535)
        rc, n_rows, bufs = _fit(tokens, OFF, spec, **kw)
        assert rc == want, (kw, list(bytes(spec)), rc)
        assert n_rows == 0 and _untouched(bufs), kw
        assert mbpe.lib().mbpe_last_error()
    # bad offsets
    rc, n_rows, bufs = _fit(T32, [0, 5, 3, 10], s32)
    assert (rc, n_rows) == (mbpe.ERR_ARG, 0) and _untouched(bufs)
    # more than 2^40 rows: 2^40 - 1 tokens with bos and eos in rows of 1 (only the offsets are read)
    o = np.array([0, (1 << 40) - 1], dtype=np.uint64)
    n_rows = ctypes.c_uint64(77)
    rc = mbpe.lib().mbpe_pack_fit_plan(o.ctypes.data, 1, ctypes.byref(_spec(1, bos_id=1, eos_id=2)), None, 0,
                                       ctypes.byref(n_rows), None, None)
    assert (rc, n_rows.value) == (mbpe.ERR_ARG, 0) and b"2^40 rows" in mbpe.lib().mbpe_last_error()
    # the edges are accepted, and the query answers without a device
    docs = [list(range(3)), [], list(range(7))]
    for spec, tokens, kw in ((s32, T32, {}), (_spec(4, bos_id=1, eos_id=2), T32, {}), (s16, T16, dict(ignore=65535)),
                             (s64, T32, dict(ignore=-(1 << 63)))):
        bos = None if spec.bos_id == mbpe.NO_TOKEN else spec.bos_id
        eos = None if spec.eos_id == mbpe.NO_TOKEN else spec.eos_id
        rows = len(ref_fit(docs, 4, bos, eos, 0, -1)["len"])
        rc, n_rows, bufs = _fit(tokens, OFF, spec, out=False, **kw)
        assert (rc, n_rows) == (mbpe.OK, rows) and _untouched(bufs), kw
        rc, n_rows, bufs = _fit(tokens, OFF, spec, cap=rows - 1, **kw)         # too small: the count alone
        assert (rc, n_rows) == (mbpe.ERR_ARG, rows) and _untouched(bufs), kw
        assert b"too small" in mbpe.lib().mbpe_last_error()
    # nothing to write is no device call; documents without an element say so in doc_row
    rc, n_rows, bufs = _fit(np.zeros(0, dtype=np.uint32), [0], s32)
    assert (rc, n_rows) == (mbpe.OK, 0) and _untouched(bufs)
    out = mbpe.pack_fit(np.zeros(0, dtype=np.uint32), [0], 4, out_bits=64, labels=True, positions=True, segments=True,
                        cu_seqlens=True, doc_row=True, doc_col=True)
    assert list(out) == ["ids", "lengths", "labels", "positions", "segments", "doc_row", "doc_col", "cu_seqlens", "max_seqlen"]
    assert out["ids"].shape == out["labels"].shape == (0, 4) and out["doc_row"].shape == out["doc_col"].shape == (0,)
    assert (out["labels"].dtype, out["doc_row"].dtype, out["doc_col"].dtype) == (np.int64, np.uint64, np.uint32)
    assert out["cu_seqlens"].tolist() == [0] and out["max_seqlen"] == 0
    out = mbpe.pack_fit(np.zeros(0, dtype=np.uint32), [0, 0, 0, 0], 4, doc_row=True, doc_col=True)
    assert out["ids"].shape == (0, 4) and out["doc_row"].tolist() == [NO_ROW] * 3 and out["doc_col"].tolist() == [0] * 3


def test_plan_and_cu_seqlens_argument_errors():
    L = mbpe.lib()
    o = np.array(OFF, dtype=np.uint64)
    spec = _spec(4)
    ln = np.full(8, 0xABABABAB, dtype=np.uint32)
    drow = np.full(3, 0xAB, dtype=np.uint64)
    dcol = np.full(3, 0xAB, dtype=np.uint32)
    cu = np.full(16, -7, dtype=np.int32)
    n, longest = ctypes.c_uint64(77), ctypes.c_uint32(77)
    bad = np.array([0, 5, 3, 10], dtype=np.uint64)
    for off_p, sp, n_out in ((None, spec, n), (o.ctypes.data, None, n), (o.ctypes.data, spec, None),
                             (o.ctypes.data, mbpe.pack_spec(4), n), (bad.ctypes.data, spec, n),
                             (o.ctypes.data, _spec(0), n)):
        n.value = 77
        rc = L.mbpe_pack_fit_plan(off_p, 3, ctypes.byref(sp) if sp else None, ln.ctypes.data, 8,
                                  ctypes.byref(n_out) if n_out else None, drow.ctypes.data, dcol.ctypes.data)
        assert rc == mbpe.ERR_ARG and (n_out is None or n.value == 0)
        n.value = longest.value = 77
        rc = L.mbpe_pack_fit_cu_seqlens(off_p, 3, ctypes.byref(sp) if sp else None, cu.ctypes.data, 15,
                                        ctypes.byref(n_out) if n_out else None, ctypes.byref(longest))
        assert rc == mbpe.ERR_ARG and (n_out is None or (n.value, longest.value) == (0, 0))
    assert L.mbpe_pack_fit_cu_seqlens(o.ctypes.data, 3, ctypes.byref(spec), cu.ctypes.data, 15, ctypes.byref(n), None) == mbpe.ERR_ARG
    # T = 3, 0, 7 in rows of 4: [the full piece of document 2] [document 0 . pad] [the tail of document 2 . pad]
    rc = L.mbpe_pack_fit_plan(o.ctypes.data, 3, ctypes.byref(spec), ln.ctypes.data, 2, ctypes.byref(n), drow.ctypes.data,
                              dcol.ctypes.data)
    assert (rc, n.value) == (mbpe.ERR_ARG, 3) and b"too small" in L.mbpe_last_error()
    rc = L.mbpe_pack_fit_cu_seqlens(o.ctypes.data, 3, ctypes.byref(spec), cu.ctypes.data, 4, ctypes.byref(n), ctypes.byref(longest))
    assert (rc, n.value, longest.value) == (mbpe.ERR_ARG, 5, 4) and b"too small" in L.mbpe_last_error()
    assert (ln == 0xABABABAB).all() and (drow == 0xAB).all() and (dcol == 0xAB).all() and (cu == -7).all()
    plan = mbpe.pack_fit_plan(OFF, 4)
    assert plan["n_rows"] == 3 and plan["lengths"].tolist() == [4, 3, 3]
    assert plan["doc_row"].tolist() == [1, NO_ROW, 2] and plan["doc_col"].tolist() == [0, 0, 0]
    got_cu, got_longest = mbpe.pack_fit_cu_seqlens(OFF, 4)
    assert got_cu.tolist() == [0, 4, 7, 8, 11, 12] and got_longest == 4
    # n_rows * seq_len >= 2^31
    o = np.array([0, 1 << 31], dtype=np.uint64)
    assert L.mbpe_pack_fit_cu_seqlens(o.ctypes.data, 1, ctypes.byref(_spec(1 << 11)), None, 0, ctypes.byref(n),
                                      ctypes.byref(longest)) == mbpe.ERR_ARG
    assert b"2^31" in L.mbpe_last_error()


def test_encoder_and_tokenizer_fit_entry_points_check_their_arguments():
    L = mbpe.lib()
    spec = _spec(4)
    text = np.frombuffer(b"abab", dtype=np.uint8)
    docs = np.array([0, 1], dtype=np.uint64)
    ids = np.full(16, 0xABABABAB, dtype=np.uint32)
    ln = np.full(4, 0xABABABAB, dtype=np.uint32)
    lab = np.full(16, 0xABABABAB, dtype=np.uint32)
    tok_off = np.full(4, 0xABABABAB, dtype=np.uint64)
    drow = np.full(4, 0xABABABAB, dtype=np.uint64)
    aux = mbpe.PackAux(lab.ctypes.data, None, None, -100)
    fit = mbpe.PackFit(drow.ctypes.data, None)
    n_rows, n_tok = ctypes.c_uint64(77), ctypes.c_uint64(77)
    mid = (ids.ctypes.data, 4, 0, ln.ctypes.data)
    # no encoder; aux NULL; fit NULL
    for e_aux, e_fit in ((ctypes.byref(aux), ctypes.byref(fit)), (None, ctypes.byref(fit)), (ctypes.byref(aux), None)):
        n_rows.value = n_tok.value = 77
        assert L.mbpe_encoder_encode_batch_fit(None, text.ctypes.data, 4, 0, None, 0, docs.ctypes.data, 1,
                                               ctypes.byref(spec), *mid, ctypes.byref(n_rows), ctypes.byref(n_tok),
                                               e_aux, tok_off.ctypes.data, e_fit) == mbpe.ERR_ARG
        assert (n_rows.value, n_tok.value) == (0, 0)
        n_rows.value = n_tok.value = 77
        assert L.mbpe_encoder_encode_batch_endmask_fit(None, None, 0, None, None, 0, docs.ctypes.data, 0,
                                                       ctypes.byref(spec), *mid, ctypes.byref(n_rows),
                                                       ctypes.byref(n_tok), e_aux, tok_off.ctypes.data,
                                                       e_fit) == mbpe.ERR_ARG
        assert (n_rows.value, n_tok.value) == (0, 0)
    tok = mbpe.Tokenizer("")
    tok.set_merges(np.array([[97, 98]], dtype=np.uint32))
    doc_off = np.array([0, 2, 4], dtype=np.uint64)
    head = (tok._h, text.ctypes.data, doc_off.ctypes.data, 2, 0)
    fn = L.mbpe_tok_encode_batch_fit_device
    for dev, sp, e_aux, e_fit in ((0, spec, None, fit), (0, spec, aux, None), (-1, spec, aux, fit), (0, None, aux, fit)):
        n_rows.value = 77
        assert fn(*head, dev, ctypes.byref(sp) if sp else None, *mid, ctypes.byref(n_rows), None,
                  ctypes.byref(e_aux) if e_aux else None, tok_off.ctypes.data,
                  ctypes.byref(e_fit) if e_fit else None) == mbpe.ERR_ARG
        assert n_rows.value == 0
    for a in (ids, ln, lab, tok_off, drow):
        assert (a == a.dtype.type(0xABABABAB)).all()
    tok.close()


# ---- the planner and the query against the reference ----------------------------------------------------------------------

def _random_lens(rng, S, nbe, n):
    fits = max(S - nbe, 0)
    return [rng.choice([0, 1, max(fits - 1, 0), fits, fits + 1, 2 * S, 3 * S + 1, rng.randrange(2 * S + 2)]) for _ in range(n)]


def test_plan_and_query_equal_the_reference():
    rng = random.Random(20261)
    for case in range(300):
        S = rng.choice(SEQ_LENS)
        bos, eos = rng.choice(BOS_EOS)
        nbe = (bos is not None) + (eos is not None)
        lens = _random_lens(rng, S, nbe, rng.randrange(25))
        what = (case, S, bos, eos, lens)
        placed, n_rows = ref_plan([n + nbe for n in lens], S)
        length, doc_row, doc_col = plan_outputs(placed, n_rows, len(lens))
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        plan = mbpe.pack_fit_plan(off, S, bos, eos)
        assert plan["n_rows"] == n_rows and plan["lengths"].tolist() == length, what
        assert plan["doc_row"].tolist() == doc_row and plan["doc_col"].tolist() == doc_col, what
        tokens = np.full(int(off[-1]), 7, dtype=np.uint32)
        rc, got_rows, bufs = _fit(tokens, off, _spec(S, bos_id=bos, eos_id=eos), out=False)
        assert (rc, got_rows) == (mbpe.OK, n_rows) and _untouched(bufs), what


def test_plan_of_300000_documents():
    S = 512
    rng = np.random.default_rng(3)
    lens = rng.integers(0, 2 * S + 1, 300000)
    placed, n_rows = ref_plan([int(n) + 1 for n in lens], S)                 # with eos
    length, doc_row, doc_col = plan_outputs(placed, n_rows, len(lens))
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    plan = mbpe.pack_fit_plan(off, S, eos_id=2)
    assert plan["n_rows"] == n_rows
    assert np.array_equal(plan["lengths"], np.array(length, dtype=np.uint32))
    assert np.array_equal(plan["doc_row"], np.array(doc_row, dtype=np.uint64))
    assert np.array_equal(plan["doc_col"], np.array(doc_col, dtype=np.uint32))
    # what best fit is for: next to no padding (PADDED would need 300,000 rows and cut every second document)
    assert n_rows * S - int(lens.sum() + len(lens)) < 0.001 * n_rows * S


def test_cu_seqlens_are_the_run_boundaries_of_the_reference():
    rng = random.Random(20262)
    for case in range(150):
        S = rng.choice(SEQ_LENS)
        bos, eos = rng.choice(BOS_EOS)
        nbe = (bos is not None) + (eos is not None)
        lens = _random_lens(rng, S, nbe, rng.randrange(20))
        docs = [[7] * n for n in lens]
        want, longest = cu_of(ref_fit(docs, S, bos, eos, 0, -100), S)
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        cu, got_longest = mbpe.pack_fit_cu_seqlens(off, S, bos, eos)
        assert cu.dtype == np.int32 and cu.tolist() == want and got_longest == longest, (case, S, bos, eos, lens)


@pytest.mark.skipif(_has_gpu(), reason="checks the no-device failure path")
def test_no_cpu_fallback():
    rc, n_rows, bufs = _fit(T32, OFF, _spec(4))
    assert (rc, n_rows) == (mbpe.ERR_NO_DEVICE, 3) and _untouched(bufs)
    with pytest.raises(mbpe.MbpeError) as e:
        mbpe.pack_fit(T32, OFF, 4, labels=True)
    assert e.value.code == mbpe.ERR_NO_DEVICE
    tok = mbpe.Tokenizer("")
    tok.set_merges(np.array([[97, 98]], dtype=np.uint32))
    with pytest.raises(mbpe.MbpeError) as e:
        tok.encode_batch_fit([b"abab", b"", b"ab"], 4, segments=True)
    assert e.value.code == mbpe.ERR_NO_DEVICE
    tok.close()


# ---- the planner as a stand-alone program ---------------------------------------------------------------------------------

FLAGS = {
    "plain": ["-O2"],
    "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
}


@pytest.mark.parametrize("build", sorted(FLAGS))
def test_fit_planner(build, tmp_path):
    exe = str(tmp_path / "pack_fit_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Wextra", "-Werror"] + FLAGS[build] +
                          ["-I" + os.path.join(ROOT, "minbpe-cc_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                           os.path.join(HERE, "pack_fit_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    # eleven values of seq_len, nb + ne 0 .. 2, twelve lists each
    assert r.stdout.strip().endswith("ok: %d lists, 0 failures" % (11 * 3 * 12))


# ---- the reference is the specification: its twin and its own invariants --------------------------------------------------

def _random_docs(rng, S, nbe, n):
    return [[rng.randrange(10, 60000) for _ in range(m)] for m in _random_lens(rng, S, nbe, n)]


def test_reference_equals_its_naive_twin():
    rng = random.Random(13)
    for case in range(300):
        S = rng.choice(SEQ_LENS)
        bos, eos = rng.choice(BOS_EOS)
        docs = _random_docs(rng, S, (bos is not None) + (eos is not None), rng.randrange(14))
        assert ref_fit(docs, S, bos, eos, 9, -100) == ref_fit_naive(docs, S, bos, eos, 9, -100), (case, S, bos, eos)


def test_reference_has_the_properties_the_rule_promises():
    rng = random.Random(17)
    for case in range(300):
        S = rng.choice(SEQ_LENS)
        bos, eos = rng.choice(BOS_EOS)
        nbe = (bos is not None) + (eos is not None)
        docs = _random_docs(rng, S, nbe, rng.randrange(14))
        ref = ref_fit(docs, S, bos, eos, 9, -100)
        what = (case, S, bos, eos, [len(d) for d in docs])
        E = [([bos] if bos is not None else []) + d + ([eos] if eos is not None else []) for d in docs]
        n_rows = len(ref["len"])
        # rows 0 .. F - 1 are the full pieces in document order
        full = [(d, i) for d, e in enumerate(E) for i in range(len(e) // S)]
        for r, (d, i) in enumerate(full):
            assert ref["seg"][r] == [d + 1] * S and ref["pos"][r] == list(range(i * S, (i + 1) * S)), what
        for r in range(n_rows):
            n, seg = ref["len"][r], ref["seg"][r]
            # padding only at the right end; len = cells used
            assert all(seg[:n]) and not any(seg[n:]) and ref["ids"][r][n:] == [9] * (S - n), what
            assert ref["labels"][r][n:] == [-100] * (S - n) and ref["pos"][r][n:] == [0] * (S - n), what
            # piece sizes do not increase from left to right
            runs = [len([1 for c in range(n) if seg[c] == s]) for s in dict.fromkeys(seg[:n])]
            assert runs == sorted(runs, reverse=True) and sum(runs) == n, what
        assert sum(1 for n in ref["len"] if 2 * n <= S) <= 1, what
        # each document read back by seg, ordered by pos, is E_d; a document that fits lies in one row, contiguously
        cells = {}
        for r in range(n_rows):
            for c in range(S):
                if ref["seg"][r][c]:
                    cells.setdefault(ref["seg"][r][c] - 1, []).append((ref["pos"][r][c], ref["ids"][r][c], ref["labels"][r][c], r, c))
        for d, e in enumerate(E):
            got = sorted(cells.get(d, []))
            assert [g[0] for g in got] == list(range(len(e))) and [g[1] for g in got] == e, what
            assert [g[2] for g in got] == e[1:] + [-100] * (1 if e else 0), what
            if 0 < len(e) <= S:
                assert [(g[3], g[4]) for g in got] == [(got[0][3], got[0][4] + t) for t in range(len(e))], what
            if e:
                first_of_last = got[(len(e) - 1) // S * S]
                assert (ref["doc_row"][d], ref["doc_col"][d]) == (first_of_last[3], first_of_last[4]), what
            else:
                assert (ref["doc_row"][d], ref["doc_col"][d]) == (NO_ROW, 0), what


def test_grid_lengths_cover_the_edges():
    for S, nbe in ((1, 0), (3, 2), (8, 1), (33, 2)):
        lens = grid_lengths(S, nbe)
        assert 36 <= len(lens) <= 46
        assert set([0, 1, max(S - nbe - 1, 0), max(S - nbe, 0), S - nbe + 1, 2 * S, 3 * S + 1]) <= set(lens)
        assert lens[:3] == [0, 0, 0] and lens[-2:] == [0, 0] and any(lens[i:i + 4] == [0] * 4 for i in range(3, len(lens) - 6))
