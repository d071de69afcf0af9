"""CPU tests of the window layout (mbpe_pack_windows, mbpe_encoder_encode_batch_windows,
mbpe_encoder_encode_batch_endmask_windows, mbpe_tok_encode_batch_windows_device): the symbols exist, are listed and
typed and the struct matches the header; every argument error has its code before any device call and writes nothing;
the one-shot query gives the reference's row count without a device; the host arithmetic of csrc/pack_host.h passes
its stand-alone check (tests/pack_window_check.cpp), plain and under ASan + UBSan; and the reference itself
(window_cases.ref_windows, which is the specification) has the properties the rule promises."""
import ctypes
import os
import random
import re
import subprocess

import numpy as np
import pytest

import mbpe
from conftest import ROOT
from window_cases import grid_lengths, ref_padded, ref_windows, scored

HERE = os.path.dirname(os.path.abspath(__file__))
NEW = ("mbpe_pack_windows", "mbpe_encoder_encode_batch_windows", "mbpe_encoder_encode_batch_endmask_windows")
NEW_TOK = ("mbpe_tok_encode_batch_windows_device",)


def _has_gpu():
    import torch
    return torch.cuda.is_available()


def test_exports_and_the_window_struct_match_the_headers():
    L = mbpe.lib()
    header = open(os.path.join(ROOT, "include", "mbpe.h")).read()
    declared = set(re.findall(r"MBPE_API[^;]*?\b(mbpe_\w+)\s*\(", header))
    tok_header = open(os.path.join(ROOT, "include", "mbpe_tokenizer.h")).read()
    tok_declared = set(re.findall(r"MBPE_API[^;]*?\b(mbpe_tok_\w+)\s*\(", tok_header))
    for s in NEW:
        assert s in declared and s in mbpe.EXPORTS and hasattr(L, s) and getattr(L, s).argtypes, s
    for s in NEW_TOK:
        assert s in tok_declared and s in mbpe.TOK_EXPORTS and hasattr(L, s) and getattr(L, s).argtypes, s
    # the window calls take the arguments of their counterparts, then win
    assert L.mbpe_pack_windows.argtypes[:-1] == L.mbpe_pack_tokens_aux.argtypes
    assert L.mbpe_encoder_encode_batch_windows.argtypes[:-1] == L.mbpe_encoder_encode_batch_aux.argtypes
    assert L.mbpe_encoder_encode_batch_endmask_windows.argtypes[:-1] == L.mbpe_encoder_encode_batch_endmask.argtypes
    assert L.mbpe_tok_encode_batch_windows_device.argtypes[:-1] == L.mbpe_tok_encode_batch_aux_device.argtypes
    for name in ("pack_windows", "PackWindow"):
        assert hasattr(mbpe, name), name
    assert hasattr(mbpe.Encoder, "encode_batch_windows") and hasattr(mbpe.Encoder, "encode_batch_endmask_windows")
    assert hasattr(mbpe.Tokenizer, "encode_batch_windows")
    body = re.search(r"typedef struct \{([^}]*)\} mbpe_pack_window;", header).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(\w+)\s*(\*?)\s*(\w+);", body)
    assert [(t, p) for t, p, _ in fields] == [("uint32_t", ""), ("uint32_t", ""), ("uint32_t", "*"), ("uint64_t", "*")]
    assert [n for _, _, n in fields] == [f for f, _ in mbpe.PackWindow._fields_] == \
        ["stride", "score_once", "row_doc", "row_tok0"]
    assert [t for _, t in mbpe.PackWindow._fields_] == [ctypes.c_uint32] * 2 + [ctypes.c_void_p] * 2
    assert ctypes.sizeof(mbpe.PackWindow) == 24
    assert (mbpe.PackWindow.row_doc.offset, mbpe.PackWindow.row_tok0.offset) == (8, 16)
    # the existing struct and calls are as they were
    assert ctypes.sizeof(mbpe.PackSpec) == 32 and ctypes.sizeof(mbpe.PackAux) == 32


# ---- argument errors before the device ------------------------------------------------------------------------------------

T16 = np.arange(10, dtype=np.uint16)
T32 = np.arange(10, dtype=np.uint32)
OFF = [0, 3, 3, 10]
FILL = 0xAB


def _windows(tokens, off, spec, stride=0, score_once=0, ignore=-100, aux_null=False, win_null=False, want=(1, 1, 1, 1, 1),
             out=True, cap=64, on_device=0, shift=(0, 0, 0, 0, 0, 0), n_docs=None):
    """mbpe_pack_windows as it is, into prefilled host buffers (with on_device=1 the same buffers are named as device
    memory: such a call must be refused before anything is done with them) -> (code, n_rows, the buffers)."""
    t = np.ascontiguousarray(tokens)
    o = np.ascontiguousarray(off, dtype=np.uint64)
    bufs = [np.full(8192, FILL, dtype=np.uint8) for _ in range(7)]          # ids, len, labels, pos, seg, row_doc, row_tok0
    base = [b.ctypes.data + (-b.ctypes.data) % 16 for b in bufs]           # 16-byte aligned
    ids, ln, lab, pos, seg, rdoc, rtok = base
    aux = mbpe.PackAux((lab + shift[1]) if want[0] else None, (pos + shift[2]) if want[1] else None,
                       (seg + shift[3]) if want[2] else None, ignore)
    win = mbpe.PackWindow(stride, score_once, (rdoc + shift[4]) if want[3] else None,
                          (rtok + shift[5]) if want[4] else None)
    n_rows = ctypes.c_uint64(77)
    rc = mbpe.lib().mbpe_pack_windows(
        0, t.ctypes.data if len(t) else None, len(t), t.dtype.itemsize * 8, 0, o.ctypes.data,
        len(o) - 1 if n_docs is None else n_docs, ctypes.byref(spec), (ids + shift[0]) if out else None, cap, on_device,
        ln if out else None, ctypes.byref(n_rows), None if aux_null else ctypes.byref(aux),
        None if win_null else ctypes.byref(win))
    return rc, n_rows.value, bufs


def _untouched(bufs):
    return all((b == FILL).all() for b in bufs)


def test_window_argument_errors_come_before_the_device():
    s16, s32, s64 = (mbpe.pack_spec(4, out_bits=b) for b in (16, 32, 64))
    both = mbpe.pack_spec(4, bos_id=1, eos_id=2)                            # keep 2
    cases = [
        (dict(aux_null=True), s32, T32, mbpe.ERR_ARG),
        (dict(win_null=True), s32, T32, mbpe.ERR_ARG),
        # the layout: windows are PADDED rows, padded on the right, cut from the left
        ({}, mbpe.pack_spec(4, "packed"), T32, mbpe.ERR_ARG),
        ({}, mbpe.pack_spec(4, pad_left=True), T32, mbpe.ERR_ARG),
        ({}, mbpe.pack_spec(4, trunc_left=True), T32, mbpe.ERR_ARG),
        ({}, mbpe.PackSpec(2, 4, 32, 0, mbpe.NO_TOKEN, mbpe.NO_TOKEN, 0, 0), T32, mbpe.ERR_ARG),
        # seq_len < nb + ne + 1
        ({}, mbpe.pack_spec(0), T32, mbpe.ERR_ARG),
        ({}, mbpe.pack_spec(1, bos_id=1), T32, mbpe.ERR_ARG),
        ({}, mbpe.pack_spec(2, bos_id=1, eos_id=2), T32, mbpe.ERR_ARG),
        # stride >= keep
        (dict(stride=4), s32, T32, mbpe.ERR_ARG),
        (dict(stride=2), both, T32, mbpe.ERR_ARG),
        (dict(stride=3), both, T32, mbpe.ERR_ARG),
        (dict(stride=0xFFFFFFFF), s32, T32, mbpe.ERR_ARG),
        (dict(score_once=2), s32, T32, mbpe.ERR_ARG),
        # row_doc holds the document number in 32 bits (the count is checked before the offsets are read)
        (dict(n_docs=0xFFFFFFFF), s32, T32, mbpe.ERR_ARG),
        # the rules of mbpe_pack_tokens_aux: ignore_label, alignment of device outputs
        (dict(ignore=-100), s16, T16, mbpe.ERR_VOCAB),
        (dict(ignore=65536), s16, T16, mbpe.ERR_VOCAB),
        (dict(ignore=1 << 32), s32, T32, mbpe.ERR_ARG),
        (dict(on_device=1, shift=(8, 0, 0, 0, 0, 0)), s32, T32, mbpe.ERR_ARG),
        (dict(on_device=1, shift=(0, 4, 0, 0, 0, 0)), s32, T32, mbpe.ERR_ARG),
        (dict(on_device=1, shift=(0, 0, 8, 0, 0, 0)), s64, T32, mbpe.ERR_ARG),
        (dict(on_device=1, shift=(0, 0, 0, 2, 0, 0)), s16, T16, mbpe.ERR_ARG),
        (dict(on_device=1, shift=(0, 0, 0, 0, 2, 0)), s32, T32, mbpe.ERR_ARG),
        (dict(on_device=1, shift=(0, 0, 0, 0, 0, 4)), s32, T32, mbpe.ERR_ARG),
        # the MBPE_ERR_VOCAB rules of pack_check_spec
        ({}, s16, T32, mbpe.ERR_VOCAB),
        ({}, mbpe.pack_spec(4, out_bits=16, pad_id=65536), T16, mbpe.ERR_VOCAB),
        ({}, mbpe.pack_spec(4, out_bits=16, bos_id=70000), T16, mbpe.ERR_VOCAB),
        ({}, mbpe.pack_spec(4, out_bits=8), T32, mbpe.ERR_ARG),
    ]
    for kw, spec, tokens, want in cases:
        if spec.out_bits == 16:
            kw.setdefault("ignore", 65535)
        rc, n_rows, bufs = _windows(tokens, OFF, spec, **kw)
        assert rc == want, (kw, list(bytes(spec)), rc)
        assert n_rows == 0 and _untouched(bufs), kw
        assert mbpe.lib().mbpe_last_error()
    # bad offsets (the limit of 2^40 rows needs no array only in pack_window_check.cpp, which has it)
    rc, n_rows, bufs = _windows(T32, [0, 5, 3, 10], s32)
    assert (rc, n_rows) == (mbpe.ERR_ARG, 0) and _untouched(bufs)
    # the edges are accepted, and the query answers without a device: stride keep - 1, score_once 1
    for spec, tokens, kw in ((s32, T32, dict(stride=3, score_once=1)), (both, T32, dict(stride=1)),
                             (s16, T16, dict(ignore=65535, stride=3)), (s64, T32, dict(ignore=-(1 << 63)))):
        docs = [list(range(3)), [], list(range(7))]
        nb = (spec.bos_id != mbpe.NO_TOKEN) + (spec.eos_id != mbpe.NO_TOKEN)
        rows = len(ref_windows(docs, 4, kw.get("stride", 0), 1 if nb else None, 2 if nb else None, 0, -1, 0)["len"])
        rc, n_rows, bufs = _windows(tokens, OFF, spec, out=False, **kw)
        assert (rc, n_rows) == (mbpe.OK, rows) and _untouched(bufs), kw
        rc, n_rows, bufs = _windows(tokens, OFF, spec, cap=rows - 1, **kw)      # too small: the count alone
        assert (rc, n_rows) == (mbpe.ERR_ARG, rows) and _untouched(bufs), kw
        assert b"too small" in mbpe.lib().mbpe_last_error()
    # nothing to write is no device call
    rc, n_rows, bufs = _windows(np.zeros(0, dtype=np.uint32), [0], s32)
    assert (rc, n_rows) == (mbpe.OK, 0) and _untouched(bufs)
    out = mbpe.pack_windows(np.zeros(0, dtype=np.uint32), [0], 4, 1, out_bits=64, labels=True, positions=True,
                            segments=True, row_doc=True, row_tok0=True)
    assert list(out) == ["ids", "lengths", "labels", "positions", "segments", "row_doc", "row_tok0"]
    assert out["ids"].shape == out["labels"].shape == (0, 4) and out["row_doc"].shape == out["row_tok0"].shape == (0,)
    assert (out["labels"].dtype, out["row_doc"].dtype, out["row_tok0"].dtype) == (np.int64, np.uint32, np.uint64)


def test_encoder_and_tokenizer_window_entry_points_check_their_arguments():
    L = mbpe.lib()
    spec = mbpe.pack_spec(4)
    text = np.frombuffer(b"abab", dtype=np.uint8)
    docs = np.array([0, 1], dtype=np.uint64)
    ids = np.full(16, 0xABABABAB, dtype=np.uint32)
    ln = np.full(4, 0xABABABAB, dtype=np.uint32)
    lab = np.full(16, 0xABABABAB, dtype=np.uint32)
    tok_off = np.full(4, 0xABABABAB, dtype=np.uint64)
    aux = mbpe.PackAux(lab.ctypes.data, None, None, -100)
    win = mbpe.PackWindow(1, 0, None, None)
    n_rows, n_tok = ctypes.c_uint64(77), ctypes.c_uint64(77)
    mid = (ids.ctypes.data, 4, 0, ln.ctypes.data)
    # no encoder; aux NULL; win NULL
    for e_aux, e_win in ((ctypes.byref(aux), ctypes.byref(win)), (None, ctypes.byref(win)), (ctypes.byref(aux), None)):
        n_rows.value = n_tok.value = 77
        assert L.mbpe_encoder_encode_batch_windows(None, text.ctypes.data, 4, 0, None, 0, docs.ctypes.data, 1,
                                                   ctypes.byref(spec), *mid, ctypes.byref(n_rows), ctypes.byref(n_tok),
                                                   e_aux, tok_off.ctypes.data, e_win) == mbpe.ERR_ARG
        assert (n_rows.value, n_tok.value) == (0, 0)
        n_rows.value = n_tok.value = 77
        assert L.mbpe_encoder_encode_batch_endmask_windows(None, None, 0, None, None, 0, docs.ctypes.data, 0,
                                                           ctypes.byref(spec), *mid, ctypes.byref(n_rows),
                                                           ctypes.byref(n_tok), e_aux, tok_off.ctypes.data,
                                                           e_win) == mbpe.ERR_ARG
        assert (n_rows.value, n_tok.value) == (0, 0)
    tok = mbpe.Tokenizer("")
    tok.set_merges(np.array([[97, 98]], dtype=np.uint32))
    doc_off = np.array([0, 2, 4], dtype=np.uint64)
    head = (tok._h, text.ctypes.data, doc_off.ctypes.data, 2, 0)
    fn = L.mbpe_tok_encode_batch_windows_device
    for dev, sp, e_aux, e_win in ((0, spec, None, win), (0, spec, aux, None), (-1, spec, aux, win), (0, None, aux, win)):
        n_rows.value = 77
        assert fn(*head, dev, ctypes.byref(sp) if sp else None, *mid, ctypes.byref(n_rows), None,
                  ctypes.byref(e_aux) if e_aux else None, tok_off.ctypes.data,
                  ctypes.byref(e_win) if e_win else None) == mbpe.ERR_ARG
        assert n_rows.value == 0
    for a in (ids, ln, lab, tok_off):
        assert (a == a.dtype.type(0xABABABAB)).all()
    tok.close()


def test_the_query_gives_the_reference_row_count_without_a_device():
    rng = random.Random(20251)
    for case in range(200):
        seq_len = rng.choice([1, 2, 3, 4, 5, 8, 13, 16, 64])
        bos, eos = rng.choice([(None, None), (5, None), (None, 6), (5, 6)])
        nbe = (bos is not None) + (eos is not None)
        if seq_len < nbe + 1:
            seq_len = nbe + 1
        keep = seq_len - nbe
        stride = rng.randrange(keep)
        lens = [rng.choice([0, 1, keep - 1, keep, keep + 1, rng.randrange(6 * keep + 2)]) for _ in range(rng.randrange(12))]
        docs = [[7] * n for n in lens]
        want = len(ref_windows(docs, seq_len, stride, bos, eos, 0, -100, 0)["len"])
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        tokens = np.full(int(off[-1]), 7, dtype=np.uint32)
        spec = mbpe.pack_spec(seq_len, bos_id=bos, eos_id=eos)
        rc, n_rows, bufs = _windows(tokens, off, spec, stride=stride, out=False)
        assert (rc, n_rows) == (mbpe.OK, want) and _untouched(bufs), (case, seq_len, stride, bos, eos, lens)


@pytest.mark.skipif(_has_gpu(), reason="checks the no-device failure path")
def test_no_cpu_fallback():
    rc, n_rows, bufs = _windows(T32, OFF, mbpe.pack_spec(4), stride=1)
    assert (rc, n_rows) == (mbpe.ERR_NO_DEVICE, 4) and _untouched(bufs)
    with pytest.raises(mbpe.MbpeError) as e:
        mbpe.pack_windows(T32, OFF, 4, 1, labels=True)
    assert e.value.code == mbpe.ERR_NO_DEVICE
    tok = mbpe.Tokenizer("")
    tok.set_merges(np.array([[97, 98]], dtype=np.uint32))
    with pytest.raises(mbpe.MbpeError) as e:
        tok.encode_batch_windows([b"abab", b"", b"ab"], 4, 1, segments=True)
    assert e.value.code == mbpe.ERR_NO_DEVICE
    tok.close()


# ---- the host arithmetic as a stand-alone program ------------------------------------------------------------------------

FLAGS = {
    "plain": ["-O2"],
    "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
}


@pytest.mark.parametrize("build", sorted(FLAGS))
def test_window_host_arithmetic(build, tmp_path):
    exe = str(tmp_path / "pack_window_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Wextra", "-Werror"] + FLAGS[build] +
                          ["-I" + os.path.join(ROOT, "minbpe-cc_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                           os.path.join(HERE, "pack_window_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    # per seq_len and nb + ne < min(3, seq_len): one list per stride below keep
    n_lists = sum(s - nbe for s in (1, 2, 3, 4, 5, 7, 8, 9, 16) for nbe in range(min(3, s)))
    assert r.stdout.strip().endswith("ok: %d lists, 0 failures" % n_lists)


# ---- the reference is the specification: its own invariants ---------------------------------------------------------------

def _random_docs(rng, keep, n):
    return [[rng.randrange(10, 60000) for _ in range(rng.choice([0, 1, keep - 1, keep, keep + 1, rng.randrange(5 * keep + 2)]))]
            for _ in range(n)]


def test_reference_scores_every_target_exactly_once():
    rng = random.Random(7)
    for case in range(300):
        seq_len = rng.choice([3, 4, 5, 8, 13, 16])
        bos, eos = rng.choice([(None, None), (1, None), (None, 2), (1, 2)])
        keep = seq_len - (bos is not None) - (eos is not None)
        stride = rng.randrange(keep)
        docs = _random_docs(rng, keep, rng.randrange(1, 8))
        ref = ref_windows(docs, seq_len, stride, bos, eos, 0, -100, 1)
        got = scored(ref, -100)
        for d, tok in enumerate(docs):
            want = (tok if bos is not None else tok[1:]) + ([eos] if eos is not None else [])
            if not tok and bos is None:
                want = []                                    # a row of eos alone: no cell stands before it
            assert got.get(d, []) == want, (case, seq_len, stride, bos, eos, d, len(tok))
        # and without score_once the only difference is the shared cells
        plain = ref_windows(docs, seq_len, stride, bos, eos, 0, -100, 0)
        for k in ("ids", "pos", "seg", "len", "row_doc", "row_tok0"):
            assert plain[k] == ref[k]
        # the rows of a document tile its tokens: joined without the shared tokens they give the document back
        nb = int(bos is not None)
        for d, tok in enumerate(docs):
            rows = [r for r, dd in enumerate(ref["row_doc"]) if dd == d]
            assert rows == list(range(rows[0], rows[0] + len(rows)))
            joined = []
            for n, r in enumerate(rows):
                last = n == len(rows) - 1
                body = ref["ids"][r][nb:ref["len"][r] - (1 if eos is not None and last else 0)]
                assert ref["row_tok0"][r] == n * (keep - stride)
                joined += body[stride if n else 0:]
            assert joined == tok


def test_reference_equals_padded_when_every_document_fits():
    rng = random.Random(11)
    for case in range(100):
        seq_len = rng.choice([3, 4, 5, 8, 13])
        bos, eos = rng.choice([(None, None), (1, None), (None, 2), (1, 2)])
        keep = seq_len - (bos is not None) - (eos is not None)
        docs = [[rng.randrange(10, 60000) for _ in range(rng.randrange(keep + 1))] for _ in range(rng.randrange(1, 9))]
        for score_once in (0, 1):
            ref = ref_windows(docs, seq_len, rng.randrange(keep), bos, eos, 9, -100, score_once)
            pad = ref_padded(docs, seq_len, bos, eos, 9, -100)
            for k in pad:
                assert ref[k] == pad[k], (case, k)
            assert ref["row_doc"] == list(range(len(docs))) and ref["row_tok0"] == [0] * len(docs)


def test_grid_lengths_cover_the_edges():
    for keep, step in ((1, 1), (3, 1), (8, 8), (14, 13)):
        lens = grid_lengths(keep, step)
        assert 38 <= len(lens) <= 50
        assert set([0, 1, keep - 1, keep, keep + 1, keep + step - 1, keep + step, keep + step + 1, 3000]) <= set(lens)
        assert lens[:3] == [0, 0, 0] and lens[-2:] == [0, 0] and any(lens[i:i + 4] == [0] * 4 for i in range(3, len(lens) - 6))
