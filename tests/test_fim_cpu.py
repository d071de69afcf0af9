"""CPU tests of fill-in-the-middle (mbpe_fim_plan, mbpe_fim_tokens, mbpe_encoder_set_fim, mbpe_encoder_fim_info,
mbpe_tok_set_encode_fim, mbpe_tok_encode_fim_info): the symbols exist, are listed and typed and the struct matches the
header; every argument error has its code before any device call and writes nothing; the host's plan and the one-shot
query equal the reference (fim_cases.ref_plan, which restates the rule) without a device; csrc/fim.h passes its
stand-alone check (tests/fim_check.cpp), plain and under ASan + UBSan; and the reference itself has the properties the
rule promises."""
import ctypes
import os
import random
import re
import subprocess

import numpy as np
import pytest

import mbpe
from conftest import ROOT
import fim_cases as F

HERE = os.path.dirname(os.path.abspath(__file__))
NEW = ("mbpe_fim_plan", "mbpe_fim_tokens", "mbpe_fim_kernel_ms", "mbpe_encoder_set_fim", "mbpe_encoder_fim_info")
NEW_TOK = ("mbpe_tok_set_encode_fim", "mbpe_tok_encode_fim_info")
FILL, FILL64 = 0xAB, 0xABABABABABABABAB


def _has_gpu():
    import torch
    return torch.cuda.is_available()


def _c(s):
    """fim_cases.spec -> mbpe.FimSpec"""
    return mbpe.FimSpec(s["rate"], s["spm"], s["seed"], s["doc_base"], s["pre"], s["suf"], s["mid"], s["min_tokens"],
                        s["max_tokens"])


def test_exports_and_the_fim_struct_match_the_headers():
    L = mbpe.lib()
    header = open(os.path.join(ROOT, "include", "mbpe.h")).read()
    declared = set(re.findall(r"MBPE_API[^;]*?\b(mbpe_\w+)\s*\(", header))
    tok_header = open(os.path.join(ROOT, "include", "mbpe_tokenizer.h")).read()
    tok_declared = set(re.findall(r"MBPE_API[^;]*?\b(mbpe_tok_\w+)\s*\(", tok_header))
    for s in NEW:
        assert s in declared and s in mbpe.EXPORTS and hasattr(L, s) and getattr(L, s).argtypes, s
    for s in NEW_TOK:
        assert s in tok_declared and s in mbpe.TOK_EXPORTS and hasattr(L, s) and getattr(L, s).argtypes, s
    # mbpe_fim_tokens has the conventions of mbpe_pack_tokens up to the spec, and of mbpe_unpack_tokens behind it
    assert L.mbpe_fim_tokens.argtypes[:8] == L.mbpe_pack_tokens.argtypes[:8]
    assert len(L.mbpe_fim_tokens.argtypes) == 13 and len(L.mbpe_fim_plan.argtypes) == 6
    assert L.mbpe_encoder_fim_info.argtypes == L.mbpe_tok_encode_fim_info.argtypes
    assert len(L.mbpe_encoder_fim_info.argtypes) == 5
    assert L.mbpe_encoder_set_fim.argtypes == L.mbpe_tok_set_encode_fim.argtypes == [ctypes.c_void_p] * 2
    for name in ("FimSpec", "fim_spec", "fim_plan", "fim_tokens", "fim_kernel_ms"):
        assert hasattr(mbpe, name), name
    assert hasattr(mbpe.Encoder, "set_fim") and hasattr(mbpe.Encoder, "fim_info") and hasattr(mbpe.Tokenizer, "fim_info")
    import inspect
    for m in ("encode_batch_padded", "encode_batch_aux", "encode_batch_windows", "encode_batch_fit"):
        assert inspect.signature(getattr(mbpe.Tokenizer, m)).parameters["fim"].default is None, m
    body = re.search(r"typedef struct \{([^}]*)\} mbpe_fim_spec;", header).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for typ, names in re.findall(r"(uint\d+_t)\s+([^;]+);", body):
        fields += [(n.strip(), typ) for n in names.split(",")]
    ctype = {"uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32}
    assert [(n, ctype[t]) for n, t in fields] == list(mbpe.FimSpec._fields_)
    assert [n for n, _ in fields] == ["rate", "spm", "seed", "doc_base", "pre_id", "suf_id", "mid_id", "min_tokens",
                                      "max_tokens"]
    assert ctypes.sizeof(mbpe.FimSpec) == 56 and mbpe.FimSpec.pre_id.offset == 32 and mbpe.FimSpec.max_tokens.offset == 48
    sp = mbpe.fim_spec(0.5, 1.0, 7, 8, 9, seed=-1, doc_base=1 << 40, min_tokens=2, max_tokens=5)
    assert (sp.rate, sp.spm, sp.seed, sp.doc_base) == (1 << 31, 1 << 32, (1 << 64) - 1, 1 << 40)
    assert (sp.pre_id, sp.suf_id, sp.mid_id, sp.min_tokens, sp.max_tokens) == (7, 8, 9, 2, 5)
    with pytest.raises(mbpe.MbpeError):
        mbpe.fim_spec(1.5, 0, 1, 2, 3)


# ---- argument errors before the device ------------------------------------------------------------------------------------

T16 = np.arange(10, dtype=np.uint16)
T32 = np.arange(10, dtype=np.uint32)
OFF = [0, 3, 3, 10]


def _tokens(tokens, off, spec, out=True, cap=64, on_device=0, shift=0, spec_null=False, n_null=False, bits=None):
    """mbpe_fim_tokens as it is, into prefilled host buffers (with on_device=1 the same buffer is named as device
    memory: such a call must be refused before anything is done with it) -> (code, n_out, the buffers)."""
    t = np.ascontiguousarray(tokens)
    o = np.ascontiguousarray(off, dtype=np.uint64)
    bufs = [np.full(1024, FILL, dtype=np.uint8), np.full(16, FILL64, dtype=np.uint64)]   # tokens, offsets
    base = [bufs[0].ctypes.data + (-bufs[0].ctypes.data) % 16, bufs[1].ctypes.data]
    n = ctypes.c_uint64(77)
    rc = mbpe.lib().mbpe_fim_tokens(
        0, t.ctypes.data if len(t) else None, len(t), bits or t.dtype.itemsize * 8, 0, o.ctypes.data, len(o) - 1,
        None if spec_null else ctypes.byref(spec), (base[0] + shift) if out else None, cap, on_device, base[1],
        None if n_null else ctypes.byref(n))
    return rc, n.value, bufs


def _untouched(bufs):
    return all((b.view(np.uint8) == FILL).all() for b in bufs)


def test_fim_argument_errors_come_before_the_device():
    ok = _c(F.spec())
    cases = [
        (dict(spec_null=True), ok, T32, mbpe.ERR_ARG),
        (dict(n_null=True), ok, T32, mbpe.ERR_ARG),
        (dict(bits=8), ok, T32, mbpe.ERR_ARG),
        ({}, _c(F.spec(rate=F.ONE + 1)), T32, mbpe.ERR_ARG),
        ({}, _c(F.spec(spm=F.ONE + 1)), T32, mbpe.ERR_ARG),
        ({}, _c(F.spec(min_tokens=5, max_tokens=4)), T32, mbpe.ERR_ARG),
        ({}, _c(F.spec(pre=0x7FFFFFFE)), T32, mbpe.ERR_ARG),
        ({}, _c(F.spec(suf=0xFFFFFFFF)), T32, mbpe.ERR_ARG),
        ({}, _c(F.spec(mid=0x7FFFFFFE)), T16, mbpe.ERR_ARG),
        ({}, _c(F.spec(pre=65536)), T16, mbpe.ERR_VOCAB),
        ({}, _c(F.spec(mid=0x7FFFFFFD)), T16, mbpe.ERR_VOCAB),
        (dict(on_device=1, shift=2), ok, T32, mbpe.ERR_ARG),
        (dict(on_device=1, shift=1), ok, T16, mbpe.ERR_ARG),
    ]
    for kw, spec, tokens, want in cases:
        rc, n, bufs = _tokens(tokens, OFF, spec, **kw)
        assert rc == want, (kw, list(bytes(spec)), rc)
        assert _untouched(bufs), kw
        assert kw.get("n_null") or n == (16 if kw.get("on_device") else 0), kw     # (the count comes before the address)
        assert mbpe.lib().mbpe_last_error()
    # bad offsets: descending, not from 0, not to n_tokens
    for bad in ([0, 5, 3, 10], [1, 3, 3, 10], [0, 3, 3, 9]):
        rc, n, bufs = _tokens(T32, bad, ok)
        assert (rc, n) == (mbpe.ERR_ARG, 0) and _untouched(bufs)
    # a document of 2^32 - 1 tokens or more, with rate > 0: named (only the offsets are read by the plan and the query)
    L = mbpe.lib()
    o = np.array([0, 4, 4 + (1 << 32) - 1, 7 + (1 << 32)], dtype=np.uint64)
    out = np.full(4, 77, dtype=np.uint64)
    mode = np.full(3, FILL, dtype=np.uint8)
    cut = np.full(6, 77, dtype=np.uint64)
    tiny = _c(F.spec(rate=1, max_tokens=10))
    assert L.mbpe_fim_plan(o.ctypes.data, 3, ctypes.byref(tiny), out.ctypes.data, mode.ctypes.data,
                           cut.ctypes.data) == mbpe.ERR_ARG
    assert b"document 1 " in L.mbpe_last_error()
    assert (out == 77).all() and (mode == FILL).all() and (cut == 77).all()
    o[2] -= 1                                                    # 2^32 - 2 is the longest there is
    assert L.mbpe_fim_plan(o.ctypes.data, 3, ctypes.byref(_c(F.spec())), out.ctypes.data, mode.ctypes.data,
                           cut.ctypes.data) == mbpe.OK
    want_off, want_mode, want_cut = F.ref_plan(np.diff(o).tolist(), F.spec())
    assert (out.tolist(), mode.tolist(), cut.reshape(-1, 2).tolist()) == (want_off, want_mode, want_cut)
    assert want_mode[1] != F.NONE and want_cut[1][1] <= (1 << 32) - 2
    o[2] += 1
    assert L.mbpe_fim_plan(o.ctypes.data, 3, ctypes.byref(_c(F.spec(rate=0))), out.ctypes.data, None, None) == mbpe.OK
    assert out.tolist() == o.tolist()
    # the plan's own NULLs and spec
    for off_p, sp, out_p in ((None, ok, out), (o.ctypes.data, None, out), (o.ctypes.data, ok, None),
                             (o.ctypes.data, _c(F.spec(rate=F.ONE + 1)), out)):
        before = out.copy()
        assert L.mbpe_fim_plan(off_p, 3, ctypes.byref(sp) if sp else None, out_p.ctypes.data if out_p is not None else None,
                               None, None) == mbpe.ERR_ARG
        assert (out == before).all()
    ms = ctypes.c_float(5)
    assert L.mbpe_fim_kernel_ms(None) == mbpe.ERR_ARG and L.mbpe_fim_kernel_ms(ctypes.byref(ms)) == mbpe.OK
    # the encoder's and the tokenizer's entry points without a handle
    n = ctypes.c_uint64(77)
    assert L.mbpe_encoder_set_fim(None, ctypes.byref(ok)) == mbpe.ERR_ARG
    assert L.mbpe_encoder_fim_info(None, None, None, 0, ctypes.byref(n)) == mbpe.ERR_ARG and n.value == 77
    assert L.mbpe_tok_set_encode_fim(None, ctypes.byref(ok)) == mbpe.ERR_ARG
    assert L.mbpe_tok_encode_fim_info(None, None, None, 0, ctypes.byref(n)) == mbpe.ERR_ARG
    tok = mbpe.Tokenizer("")
    assert L.mbpe_tok_set_encode_fim(tok._h, ctypes.byref(_c(F.spec(rate=F.ONE + 1)))) == mbpe.ERR_ARG
    assert L.mbpe_tok_set_encode_fim(tok._h, ctypes.byref(_c(F.spec(suf=0x7FFFFFFE)))) == mbpe.ERR_ARG
    assert L.mbpe_tok_set_encode_fim(tok._h, ctypes.byref(ok)) == mbpe.OK
    assert L.mbpe_tok_set_encode_fim(tok._h, None) == mbpe.OK
    assert L.mbpe_tok_encode_fim_info(tok._h, None, None, 0, None) == mbpe.ERR_ARG
    assert L.mbpe_tok_encode_fim_info(tok._h, None, None, 0, ctypes.byref(n)) == mbpe.OK and n.value == 0
    mode, cuts = tok.fim_info()
    assert mode.shape == (0,) and cuts.shape == (0, 2)
    tok.close()


# ---- the plan and the query against the reference -----------------------------------------------------------------------

def test_plan_equals_the_reference_over_the_grid():
    n_cases = 0
    for n_docs in F.GRID_N_DOCS:
        lens = F.grid_lens(n_docs)
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        for rate in F.GRID_RATES:
            for spm in F.GRID_RATES:
                for lo, hi in F.GRID_LIMITS:
                    for base in F.GRID_BASES:
                        s = F.spec(F.threshold(rate), F.threshold(spm), seed=3 + n_docs, doc_base=base, min_tokens=lo,
                                   max_tokens=hi)
                        want_off, want_mode, want_cut = F.ref_plan(lens, s)
                        new_off, mode, cuts = mbpe.fim_plan(off, _c(s))
                        assert new_off.tolist() == want_off, (n_docs, s)
                        assert mode.tolist() == want_mode and cuts.tolist() == want_cut, (n_docs, s)
                        assert mode.shape == (n_docs,) and cuts.shape == (n_docs, 2)
                        n_cases += 1
    assert n_cases == 7 * 3 * 3 * 4 * 2
    if len(lens) > 40:                                           # the grid holds every length, and all three modes
        assert set(lens) == set(range(41))
    s = F.spec(F.threshold(0.5), F.threshold(0.5), seed=3)
    assert set(F.ref_plan(F.grid_lens(2049), s)[1]) == {F.NONE, F.PSM, F.SPM}
    # the library's thresholds are the reference's
    for p in (0.0, 0.25, 0.5, 1.0):
        assert mbpe.dropout_threshold(p) == F.threshold(p)


def test_query_answers_without_a_device():
    for tokens in (T16, T32):
        for s in (F.spec(), F.spec(rate=0), F.spec(min_tokens=4), F.spec(seed=9, doc_base=5)):
            want_off, _, _ = F.ref_plan([3, 0, 7], s)
            rc, n, bufs = _tokens(tokens, OFF, _c(s), out=False)
            assert (rc, n) == (mbpe.OK, want_off[-1]) and _untouched(bufs[:1])
            assert bufs[1][:4].tolist() == want_off and _untouched([bufs[1][4:]])
            rc, n, bufs = _tokens(tokens, OFF, _c(s), cap=want_off[-1] - 1)   # too small: the count alone
            assert (rc, n) == (mbpe.ERR_ARG, want_off[-1]) and _untouched(bufs)
            assert b"too small" in mbpe.lib().mbpe_last_error()
    # nothing to write is no device call
    rc, n, bufs = _tokens(np.zeros(0, dtype=np.uint32), [0, 0, 0], _c(F.spec()))
    assert (rc, n) == (mbpe.OK, 0) and _untouched(bufs[:1])
    got, off = mbpe.fim_tokens(np.zeros(0, dtype=np.uint16), [0], _c(F.spec()))
    assert got.shape == (0,) and got.dtype == np.uint16 and off.tolist() == [0]


@pytest.mark.skipif(_has_gpu(), reason="checks the no-device failure path")
def test_no_cpu_fallback():
    rc, n, bufs = _tokens(T32, OFF, _c(F.spec()))
    assert (rc, n) == (mbpe.ERR_NO_DEVICE, 16) and _untouched(bufs)
    with pytest.raises(mbpe.MbpeError) as e:
        mbpe.fim_tokens(T16, OFF, _c(F.spec(rate=0)))
    assert e.value.code == mbpe.ERR_NO_DEVICE
    tok = mbpe.Tokenizer("")
    tok.set_merges(np.array([[97, 98]], dtype=np.uint32))
    with pytest.raises(mbpe.MbpeError) as e:
        tok.encode_batch_padded([b"abab", b"", b"ab"], 8, fim=mbpe.fim_spec(1, 0.5, 300, 301, 302))
    assert e.value.code == mbpe.ERR_NO_DEVICE
    tok.close()


# ---- fim.h as a stand-alone program ---------------------------------------------------------------------------------------

FLAGS = {
    "plain": ["-O2"],
    "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
}


@pytest.mark.parametrize("build", sorted(FLAGS))
def test_fim_rule(build, tmp_path):
    exe = str(tmp_path / "fim_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Wextra", "-Werror"] + FLAGS[build] +
                          ["-I" + os.path.join(ROOT, "minbpe-cc_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                           os.path.join(HERE, "fim_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert re.search(r"ok: \d+ checks, 0 failures\s*$", r.stdout)


# ---- the reference is the specification: its own invariants ---------------------------------------------------------------

def test_reference_round_trips():
    rng = random.Random(11)
    for case in range(300):
        lens = [rng.choice([0, 1, 2, 3, rng.randrange(0, 60)]) for _ in range(rng.randrange(1, 8))]
        docs = F.docs_of_lens(lens, rng)
        s = F.spec(F.threshold(rng.choice([0.5, 1.0])), F.threshold(rng.choice([0.0, 0.5, 1.0])), seed=case,
                   doc_base=rng.choice([0, 1 << 40, F.M64]))
        new = F.ref_apply(docs, s)
        off, modes, cuts = F.ref_plan(lens, s)
        assert [len(t) for t in new] == [b - a for a, b in zip(off[:-1], off[1:])]
        assert F.ref_unapply(new, lens, s) == docs, (case, lens)
        for t, d, m, (a, b) in zip(new, docs, modes, cuts):
            if m == F.NONE:
                assert t == d
            else:
                assert t[0] == F.PRE and sorted(t) == sorted(d + [F.PRE, F.SUF, F.MID])
                assert t.index(F.SUF) == (1 + a if m == F.PSM else 1)
                assert t.index(F.MID) - t.index(F.SUF) - 1 == len(d) - b     # the suffix stands between them


def test_reference_composes_over_batches():
    rng = random.Random(5)
    docs = F.docs_of_lens([rng.randrange(0, 30) for _ in range(200)], rng)
    s = F.spec(F.threshold(0.5), F.threshold(0.5), seed=21, doc_base=1000)
    whole = F.ref_apply(docs, s)
    for k in (0, 1, 63, 64, 199, 200):
        assert F.ref_apply(docs[k:], dict(s, doc_base=1000 + k)) == whole[k:]
    assert F.ref_apply(docs, dict(s, seed=22)) != whole


def test_reference_draws_are_spread():
    lens = [10] * 4096
    _, modes, cuts = F.ref_plan(lens, F.spec(F.ONE, F.threshold(0.5), seed=7))
    assert len({(a, b) for a, b in cuts}) == 66                  # every a <= b in [0, 10]
    spm_share = modes.count(F.SPM) / 4096
    _, modes_half, _ = F.ref_plan(lens, F.spec(F.threshold(0.5), F.threshold(0.5), seed=7))
    done_share = sum(m != F.NONE for m in modes_half) / 4096
    print("spm share %.3f, transformed share %.3f" % (spm_share, done_share))
    assert 0.45 <= spm_share <= 0.55 and 0.45 <= done_share <= 0.55
