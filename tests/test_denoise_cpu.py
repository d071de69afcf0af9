"""CPU tests of span corruption (mbpe_denoise_plan, mbpe_denoise_tokens, mbpe_encoder_encode_batch_denoise,
mbpe_encoder_encode_batch_endmask_denoise, mbpe_tok_encode_batch_denoise_device): the symbols exist, are listed and typed
and the struct matches the header; every argument error has its code before any device call and writes nothing; the
host's plan and the one-shot query equal the reference (denoise_cases, which restates the rule) without a device;
csrc/denoise.h passes its stand-alone check (tests/denoise_check.cpp), plain and under ASan + UBSan; and the reference
itself has the properties the rule promises."""
import ctypes
import os
import random
import re
import subprocess

import numpy as np
import pytest

import mbpe
from conftest import ROOT
import denoise_cases as D

HERE = os.path.dirname(os.path.abspath(__file__))
NEW = ("mbpe_denoise_plan", "mbpe_denoise_tokens", "mbpe_denoise_kernel_ms", "mbpe_encoder_encode_batch_denoise",
       "mbpe_encoder_encode_batch_endmask_denoise")
NEW_TOK = ("mbpe_tok_encode_batch_denoise_device",)
FILL, FILL64 = 0xAB, 0xABABABABABABABAB


def _has_gpu():
    import torch
    return torch.cuda.is_available()


def _c(s):
    """denoise_cases.spec -> mbpe.DenoiseSpec"""
    return mbpe.DenoiseSpec(s["density"], s["seed"], s["doc_base"], s["mean_q8"], s["seg"], s["min_tokens"], s["sent"],
                            s["down"], s["n_sent"])


def test_exports_and_the_denoise_structs_match_the_headers():
    L = mbpe.lib()
    header = open(os.path.join(ROOT, "include", "mbpe.h")).read()
    declared = set(re.findall(r"MBPE_API[^;]*?\b(mbpe_\w+)\s*\(", header))
    tok_header = open(os.path.join(ROOT, "include", "mbpe_tokenizer.h")).read()
    tok_declared = set(re.findall(r"MBPE_API[^;]*?\b(mbpe_tok_\w+)\s*\(", tok_header))
    for s in NEW:
        assert s in declared and s in mbpe.EXPORTS and hasattr(L, s) and getattr(L, s).argtypes, s
    for s in NEW_TOK:
        assert s in tok_declared and s in mbpe.TOK_EXPORTS and hasattr(L, s) and getattr(L, s).argtypes, s
    # the conventions of mbpe_pack_tokens up to the spec; the batch calls those of their _aux neighbours up to n_docs
    assert L.mbpe_denoise_tokens.argtypes[:8] == L.mbpe_pack_tokens.argtypes[:8]
    assert len(L.mbpe_denoise_tokens.argtypes) == 20 and len(L.mbpe_denoise_plan.argtypes) == 8
    assert L.mbpe_encoder_encode_batch_denoise.argtypes[:8] == L.mbpe_encoder_encode_batch_aux.argtypes[:8]
    assert L.mbpe_encoder_encode_batch_endmask_denoise.argtypes[:8] == L.mbpe_encoder_encode_batch_endmask.argtypes[:8]
    assert L.mbpe_tok_encode_batch_denoise_device.argtypes[:6] == L.mbpe_tok_encode_batch_aux_device.argtypes[:6]
    assert len(L.mbpe_encoder_encode_batch_denoise.argtypes) == 16
    assert len(L.mbpe_encoder_encode_batch_endmask_denoise.argtypes) == 16
    assert len(L.mbpe_tok_encode_batch_denoise_device.argtypes) == 14
    for name in ("DenoiseSpec", "DenoiseBatch", "denoise_spec", "denoise_plan", "denoise_tokens", "denoise_kernel_ms",
                 "denoise_segment_for"):
        assert hasattr(mbpe, name), name
    for cls, m in ((mbpe.Encoder, "encode_batch_denoise"), (mbpe.Encoder, "encode_batch_endmask_denoise"),
                   (mbpe.Tokenizer, "encode_batch_denoise")):
        assert hasattr(cls, m), m
    ctype = {"uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32, "int64_t": ctypes.c_int64}
    body = re.search(r"typedef struct \{([^}]*)\} mbpe_denoise_spec;", header).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for typ, names in re.findall(r"(uint\d+_t)\s+([^;]+);", body):
        fields += [(n.strip(), typ) for n in names.split(",")]
    assert [(n, ctype[t]) for n, t in fields] == list(mbpe.DenoiseSpec._fields_)
    assert [n for n, _ in fields] == ["density", "seed", "doc_base", "mean_span_q8", "segment_tokens", "min_tokens",
                                      "sentinel_id", "sentinel_down", "n_sentinels"]
    S = mbpe.DenoiseSpec
    assert ctypes.sizeof(S) == 48
    assert [getattr(S, n).offset for n, _ in fields] == [0, 8, 16, 24, 28, 32, 36, 40, 44]
    body = re.search(r"typedef struct \{([^}]*)\} mbpe_denoise_batch;", header).group(1)
    names = re.findall(r"\*?(\w+);", body)
    assert names == [n for n, _ in mbpe.DenoiseBatch._fields_]
    assert names == ["enc_ids", "enc_len", "dec_ids", "dec_len", "dec_labels", "row_doc", "ignore_label"]
    assert ctypes.sizeof(mbpe.DenoiseBatch) == 56 and mbpe.DenoiseBatch.ignore_label.offset == 48
    sp = mbpe.denoise_spec(0.5, 3.0, sentinel_id=32099, seed=-1, doc_base=1 << 40, segment_tokens=568, min_tokens=4)
    assert (sp.density, sp.seed, sp.doc_base) == (1 << 31, (1 << 64) - 1, 1 << 40)
    assert (sp.mean_span_q8, sp.segment_tokens, sp.min_tokens, sp.sentinel_id, sp.sentinel_down, sp.n_sentinels) == \
        (768, 568, 4, 32099, 1, 100)
    assert mbpe.denoise_spec(sentinel_id=5, sentinel_down=False).density == D.T5_DENSITY
    with pytest.raises(mbpe.MbpeError):
        mbpe.denoise_spec(1.5, sentinel_id=1)
    with pytest.raises(ValueError):
        mbpe.denoise_spec()


# ---- argument errors before the device ------------------------------------------------------------------------------------

T16 = np.arange(40, dtype=np.uint16)
T32 = np.arange(40, dtype=np.uint32)
OFF = [0, 13, 13, 40]


def _tokens(tokens, off, spec, out=True, cap_in=64, cap_tg=64, cap_units=8, on_device=0, shift_in=0, shift_tg=0,
            spec_null=False, null=None, bits=None, units=True):
    """mbpe_denoise_tokens as it is, into prefilled host buffers (with on_device=1 the same buffers are named as device
    memory: such a call must be refused before anything is done with them) -> (code, (units, in, tg), the buffers)."""
    t = np.ascontiguousarray(tokens)
    o = np.ascontiguousarray(off, dtype=np.uint64)
    bufs = [np.full(1024, FILL, dtype=np.uint8), np.full(1024, FILL, dtype=np.uint8)] + \
        [np.full(16, FILL64, dtype=np.uint64) for _ in range(3)]             # inputs, targets, in_off, tg_off, unit_doc
    base = [b.ctypes.data + (-b.ctypes.data) % 16 for b in bufs[:2]]
    n = [ctypes.c_uint64(77) for _ in range(3)]
    refs = [None if null == k else ctypes.byref(n[k]) for k in range(3)]
    rc = mbpe.lib().mbpe_denoise_tokens(
        0, t.ctypes.data if len(t) else None, len(t), bits or t.dtype.itemsize * 8, 0, o.ctypes.data, len(o) - 1,
        None if spec_null else ctypes.byref(spec), (base[0] + shift_in) if out else None, cap_in,
        (base[1] + shift_tg) if out else None, cap_tg, on_device, *[b.ctypes.data if units else None for b in bufs[2:]],
        cap_units, *refs)
    return rc, tuple(x.value for x in n), bufs


def _untouched(bufs):
    return all((b.view(np.uint8) == FILL).all() for b in bufs)


def test_denoise_argument_errors_come_before_the_device():
    ok = _c(D.spec())
    want_n = (3, D.ref_plan([13, 0, 27], D.spec())[0][-1], D.ref_plan([13, 0, 27], D.spec())[1][-1])
    cases = [
        (dict(spec_null=True), ok, T32, mbpe.ERR_ARG),
        (dict(null=0), ok, T32, mbpe.ERR_ARG),
        (dict(null=1), ok, T32, mbpe.ERR_ARG),
        (dict(null=2), ok, T32, mbpe.ERR_ARG),
        (dict(bits=8), ok, T32, mbpe.ERR_ARG),
        ({}, _c(D.spec(density=D.ONE + 1)), T32, mbpe.ERR_ARG),
        ({}, _c(D.spec(mean_q8=255)), T32, mbpe.ERR_ARG),
        ({}, _c(D.spec(n_sent=0)), T32, mbpe.ERR_ARG),
        ({}, _c(D.spec(down=2)), T32, mbpe.ERR_ARG),
        ({}, _c(D.spec(sent=98)), T32, mbpe.ERR_ARG),                         # down: 98 - 99 < 0
        ({}, _c(D.spec(sent=0x7FFFFFFE, n_sent=1)), T32, mbpe.ERR_ARG),
        ({}, _c(D.spec(sent=0x7FFFFFFD - 98, down=0)), T32, mbpe.ERR_ARG),     # up: the last one is 2^31 - 2
        ({}, _c(D.spec(sent=0xFFFFFFFF)), T16, mbpe.ERR_ARG),
        ({}, _c(D.spec(sent=65536)), T16, mbpe.ERR_VOCAB),
        ({}, _c(D.spec(sent=65535 - 98, down=0)), T16, mbpe.ERR_VOCAB),
        (dict(on_device=1, shift_in=2), ok, T32, mbpe.ERR_ARG),
        (dict(on_device=1, shift_tg=2), ok, T32, mbpe.ERR_ARG),
        (dict(on_device=1, shift_in=1), ok, T16, mbpe.ERR_ARG),
    ]
    for kw, spec, tokens, want in cases:
        rc, n, bufs = _tokens(tokens, OFF, spec, **kw)
        assert rc == want, (kw, list(bytes(spec)), rc)
        assert _untouched(bufs), kw
        if "null" not in kw:
            assert n == (want_n if kw.get("on_device") else (0, 0, 0)), kw     # (the counts come before the addresses)
        assert mbpe.lib().mbpe_last_error()
    assert _tokens(T16, OFF, _c(D.spec(sent=65535 - 99, down=0)), out=False)[0] == mbpe.OK
    assert _tokens(T32, OFF, _c(D.spec(sent=0x7FFFFFFD - 99, down=0)), out=False)[0] == mbpe.OK
    # bad offsets: descending, not from 0, not to n_tokens
    for bad in ([0, 15, 13, 40], [1, 13, 13, 40], [0, 13, 13, 39]):
        rc, n, bufs = _tokens(T32, bad, ok)
        assert (rc, n) == (mbpe.ERR_ARG, (0, 0, 0)) and _untouched(bufs)
    # a unit of 2^32 - 1 tokens or more, with density > 0: named (only the offsets are read by the plan)
    L = mbpe.lib()
    o = np.array([0, 4, 4 + (1 << 32) - 1, 7 + (1 << 32)], dtype=np.uint64)
    arrs = [np.full(5, 77, dtype=np.uint64) for _ in range(3)]
    n = ctypes.c_uint64(77)

    def plan(sp, off=o, n_ref=n, ptrs=True, cap=4):
        return L.mbpe_denoise_plan(off.ctypes.data if off is not None else None, 3, ctypes.byref(sp) if sp else None,
                                   ctypes.byref(n_ref) if n_ref is not None else None,
                                   *[a.ctypes.data if ptrs else None for a in arrs], cap)
    assert plan(_c(D.spec(density=1))) == mbpe.ERR_ARG
    assert b"document 1 " in L.mbpe_last_error() and n.value == 0
    assert all((a == 77).all() for a in arrs)
    assert plan(_c(D.spec(density=0))) == mbpe.OK and n.value == 3       # nothing is drawn: nothing is too long
    assert arrs[0].tolist()[:4] == o.tolist() and arrs[1].tolist()[:4] == [0] * 4 and arrs[2].tolist()[:3] == [0, 1, 2]
    o[2] -= 1                                                            # 2^32 - 2 is the longest there is
    s = D.spec(density=D.ONE // 2, n_sent=7)
    assert plan(_c(s)) == mbpe.OK and n.value == 3
    want = D.ref_plan(np.diff(o).tolist(), s)
    assert [a.tolist()[:len(w)] for a, w in zip(arrs, want)] == [list(w) for w in want]
    # segments of a long document: the count alone, then a cap too small
    o[2] += 1
    for a in arrs:
        a[:] = 77
    assert plan(_c(D.spec(seg=1 << 30)), ptrs=False, cap=0) == mbpe.OK and n.value == 1 + 4 + 1
    assert plan(_c(D.spec(seg=1 << 30)), cap=5) == mbpe.ERR_ARG and n.value == 6
    assert b"fewer units" in L.mbpe_last_error() and all((a == 77).all() for a in arrs)
    assert plan(_c(D.spec(seg=1000)), ptrs=False) == mbpe.OK and n.value == 2 + 4294968
    # the plan's own NULLs and spec
    for off_p, sp, n_ref in ((None, ok, n), (o, None, n), (o, ok, None), (o, _c(D.spec(mean_q8=0)), n)):
        assert plan(sp, off=off_p, n_ref=n_ref) == mbpe.ERR_ARG
        assert all((a == 77).all() for a in arrs)
    ms = ctypes.c_float(5)
    assert L.mbpe_denoise_kernel_ms(None) == mbpe.ERR_ARG and L.mbpe_denoise_kernel_ms(ctypes.byref(ms)) == mbpe.OK


def test_batch_calls_refuse_bad_arguments_without_a_handle():
    L = mbpe.lib()
    dn, es, ds = _c(D.spec()), mbpe.pack_spec(16), mbpe.pack_spec(8)
    out = mbpe.DenoiseBatch(None, None, None, None, None, None, -100)
    n_rows, n_tok = ctypes.c_uint64(77), ctypes.c_uint64(77)
    off = np.array([0, 2], dtype=np.uint64)
    text = np.frombuffer(b"ab", dtype=np.uint8)
    ref = ctypes.byref
    tail = (0, 0, ref(n_rows), ref(n_tok))
    head = (None, text.ctypes.data, 2, 0, off.ctypes.data, 1, off.ctypes.data, 1)
    fn = L.mbpe_encoder_encode_batch_denoise
    for args in ((None, ref(es), ref(ds), ref(out)), (ref(dn), None, ref(ds), ref(out)), (ref(dn), ref(es), None, ref(out)),
                 (ref(dn), ref(es), ref(ds), None), (ref(dn), ref(es), ref(ds), ref(out))):     # (the last: no encoder)
        n_rows.value = n_tok.value = 77
        assert fn(*head, *args, *tail) == mbpe.ERR_ARG
        assert (n_rows.value, n_tok.value) == (0, 0)
    fn = L.mbpe_encoder_encode_batch_endmask_denoise
    head = (None, None, 0, None, None, 0, off.ctypes.data, 0)
    for args in ((None, ref(es), ref(ds), ref(out)), (ref(dn), ref(es), None, ref(out)), (ref(dn), ref(es), ref(ds), None),
                 (ref(dn), ref(es), ref(ds), ref(out))):
        assert fn(*head, *args, *tail) == mbpe.ERR_ARG
    tok = mbpe.Tokenizer("")
    fn = L.mbpe_tok_encode_batch_denoise_device
    for t, d, e, k, o, dev in ((None, dn, es, ds, out, 0), (tok._h, None, es, ds, out, 0), (tok._h, dn, None, ds, out, 0),
                               (tok._h, dn, es, None, out, 0), (tok._h, dn, es, ds, None, 0), (tok._h, dn, es, ds, out, -1)):
        n_rows.value = 77
        rc = fn(t, text.ctypes.data, off.ctypes.data, 1, 0, dev, *[ref(x) if x is not None else None for x in (d, e, k, o)],
                0, 0, ref(n_rows), ref(n_tok))
        assert rc == mbpe.ERR_ARG and n_rows.value == 0
    tok.close()


# ---- the plan and the query against the reference -----------------------------------------------------------------------

def test_plan_equals_the_reference_over_the_grid():
    lens = D.GRID_LENS
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    n_cases = 0
    for density in D.GRID_DENSITIES:
        for mean_q8, n_sent in D.GRID_SHAPES:
            for seg in (0, 7, 568):
                for min_tokens in (0, 10):
                    s = D.spec(D.threshold(density), mean_q8, seed=3, doc_base=5, seg=seg, min_tokens=min_tokens,
                               n_sent=n_sent, sent=D.SENT)
                    want = D.ref_plan(lens, s)
                    got = mbpe.denoise_plan(off, _c(s))
                    assert [g.tolist() for g in got] == [list(w) for w in want], s
                    assert got[2].shape == (len(want[2]),)
                    n_cases += 1
    assert n_cases == 4 * 4 * 3 * 2
    for p in (0.0, 0.15, 0.5, 1.0):                              # the library's thresholds are the reference's
        assert mbpe.dropout_threshold(p) == D.threshold(p)
    assert D.T5_DENSITY == D.threshold(0.15)


def test_anchors():
    t5 = D.spec()
    assert D.counts(t5, 568) == (85, 28) and D.counts(t5, 512) == (77, 26)
    for L, n_in, n_tg in ((568, 511, 113), (512, 461, 103)):
        in_off, tg_off, unit_doc = mbpe.denoise_plan([0, L], _c(t5))
        assert (in_off.tolist(), tg_off.tolist(), unit_doc.tolist()) == ([0, n_in], [0, n_tg], [0])
    assert D.ref_unit(t5, 0, 0, list(range(20))) == (list(range(17)) + [32099], [32099, 17, 18, 19])
    lens = [0, 1, 568, 1431]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    in_off, tg_off, unit_doc = mbpe.denoise_plan(off, _c(D.spec(seg=568)))
    assert unit_doc.tolist() == [0, 1, 2, 3, 3, 3] and len(in_off) == len(tg_off) == 7
    assert mbpe.denoise_segment_for(512, 114, 0.15, 3.0) == 568
    assert mbpe.denoise_segment_for(511, 113, 0.15, 3.0, eos=False) == 568
    assert mbpe.denoise_segment_for(512, 114, 0.15, 3.0) > mbpe.denoise_segment_for(511, 114, 0.15, 3.0)
    assert mbpe.denoise_segment_for(1, 1, 0.15, 3.0) == 0 and mbpe.denoise_segment_for(2, 1, 0.15, 3.0) == 1
    # every unit up to the answer fits, and the next length does not
    for enc_len, dec_len, density, mean in ((512, 114, 0.15, 3.0), (128, 128, 0.5, 3.0), (64, 300, 0.5, 1.0)):
        seg = mbpe.denoise_segment_for(enc_len, dec_len, density, mean)
        s = D.spec(D.threshold(density), int(mean * 256))
        fits = lambda L: (L - D.counts(s, L)[0] + D.counts(s, L)[1] + 1 <= enc_len and
                          (sum(D.counts(s, L)) + 1 if D.counts(s, L)[1] else 0) <= dec_len)
        assert seg > 0 and all(fits(L) for L in range(1, seg + 1)) and not fits(seg + 1)


def test_query_answers_without_a_device():
    lens = [13, 0, 27]
    for tokens in (T16, T32):
        for s in (D.spec(), D.spec(density=0), D.spec(min_tokens=14), D.spec(seed=9, doc_base=5, seg=7),
                  D.spec(density=D.ONE, mean_q8=256)):
            want = D.ref_plan(lens, s)
            n_u = len(want[2])
            rc, n, bufs = _tokens(tokens, OFF, _c(s), out=False, cap_units=16)
            assert (rc, n) == (mbpe.OK, (n_u, want[0][-1], want[1][-1])) and _untouched(bufs[:2])
            assert bufs[2][:n_u + 1].tolist() == want[0] and bufs[3][:n_u + 1].tolist() == want[1]
            assert bufs[4][:n_u].tolist() == want[2]
            assert _untouched([bufs[2][n_u + 1:], bufs[3][n_u + 1:], bufs[4][n_u:]])
            # caps too small: the counts alone
            for kw in (dict(cap_in=want[0][-1] - 1), dict(cap_tg=want[1][-1] - 1), dict(cap_units=n_u - 1),
                       dict(cap_units=n_u - 1, out=False)):
                if kw.get("cap_tg", 0) < 0:
                    continue
                rc, n, bufs = _tokens(tokens, OFF, _c(s), **{**dict(cap_units=16), **kw})
                assert (rc, n) == (mbpe.ERR_ARG, (n_u, want[0][-1], want[1][-1])), kw
                assert _untouched(bufs), kw
            rc, n, bufs = _tokens(tokens, OFF, _c(s), out=False, units=False, cap_units=0)
            assert (rc, n) == (mbpe.OK, (n_u, want[0][-1], want[1][-1])) and _untouched(bufs)
    # nothing to write is no device call
    rc, n, bufs = _tokens(np.zeros(0, dtype=np.uint32), [0, 0, 0], _c(D.spec()))
    assert (rc, n) == (mbpe.OK, (2, 0, 0)) and _untouched(bufs[:2])
    assert bufs[2][:3].tolist() == [0, 0, 0] and bufs[4][:2].tolist() == [0, 1]
    got = mbpe.denoise_tokens(np.zeros(0, dtype=np.uint16), [0], _c(D.spec()))
    assert got[0].shape == (0,) and got[0].dtype == np.uint16 and got[1].shape == (0,)
    assert [g.tolist() for g in got[2:]] == [[0], [0], []]


@pytest.mark.skipif(_has_gpu(), reason="checks the no-device failure path")
def test_no_cpu_fallback():
    rc, n, bufs = _tokens(T32, OFF, _c(D.spec()))
    assert rc == mbpe.ERR_NO_DEVICE and n[0] == 3 and _untouched(bufs)
    with pytest.raises(mbpe.MbpeError) as e:
        mbpe.denoise_tokens(T16, OFF, _c(D.spec()))
    assert e.value.code == mbpe.ERR_NO_DEVICE
    tok = mbpe.Tokenizer("")
    tok.set_merges(np.array([[97, 98]], dtype=np.uint32))
    with pytest.raises(mbpe.MbpeError) as e:
        tok.encode_batch_denoise([b"abab", b"", b"ab"], 8, 8, mbpe.denoise_spec(0.5, sentinel_id=400))
    assert e.value.code == mbpe.ERR_NO_DEVICE
    tok.close()


# ---- denoise.h as a stand-alone program -----------------------------------------------------------------------------------

FLAGS = {
    "plain": ["-O2"],
    "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
}


@pytest.mark.parametrize("build", sorted(FLAGS))
def test_denoise_rule(build, tmp_path):
    exe = str(tmp_path / "denoise_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Wextra", "-Werror"] + FLAGS[build] +
                          ["-I" + os.path.join(ROOT, "minbpe-cc_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                           os.path.join(HERE, "denoise_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert re.search(r"ok: \d+ checks, 0 failures\s*$", r.stdout)


# ---- the reference is the specification: its own invariants ---------------------------------------------------------------

def test_reference_properties_over_the_grid():
    """Every position of both streams, the closed forms included, for L = 0 .. 39, 511, 512, 568, 1025 and 5000."""
    rng = random.Random(3)
    for L in D.GRID_LENS:
        t = [rng.randrange(30000) for _ in range(L)]
        for density in D.GRID_DENSITIES:
            for mean_q8, n_sent in D.GRID_SHAPES:
                s = D.spec(D.threshold(density), mean_q8, seed=L, n_sent=n_sent)
                N, S = D.counts(s, L)
                inp, tg = D.ref_unit(s, 4, 2, t)
                assert (len(inp), len(tg)) == ((L - N + S, N + S) if S else (L, 0)), (L, s)
                if S == 0:
                    assert inp == t and (density == 0 or L < 2)
                    continue
                assert 1 <= N <= L - 1 and 1 <= S <= min(N, L - N, n_sent)
                sent = [D.sid(s, j) for j in range(S)]
                assert [x for x in inp if x >= 30000] == sent == [x for x in tg if x >= 30000]
                # the body tokens of both streams are the unit's tokens, in order within each stream
                body_in, body_tg = [x for x in inp if x < 30000], [x for x in tg if x < 30000]
                assert sorted(body_in + body_tg) == sorted(t)
                # no two sentinels touch in the inputs; a unit begins with kept text and ends with noise
                assert all(not (a >= 30000 and b >= 30000) for a, b in zip(inp, inp[1:]))
                assert inp[0] == t[0] and inp[-1] == sent[-1] and tg[0] == sent[0] and tg[-1] == t[-1]
                # interleaving the parts gives the unit back
                back, i, g = [], 0, 1
                for j in range(S):
                    while inp[i] < 30000:
                        back.append(inp[i]); i += 1
                    i += 1
                    while g < len(tg) and tg[g] < 30000:
                        back.append(tg[g]); g += 1
                    g += 1
                assert back == t
                step = 1 if L <= 600 else 13
                assert all(D.ref_input_at(s, 4, 2, t, p) == inp[p] for p in range(0, len(inp), step))
                assert all(D.ref_target_at(s, 4, 2, t, p) == tg[p] for p in range(0, len(tg), step))


def test_reference_composes_over_batches_and_seeds():
    rng = random.Random(5)
    docs = D.docs_of_lens([rng.randrange(0, 60) for _ in range(120)], rng)
    s = D.spec(D.threshold(0.3), 512, seed=21, doc_base=1000, seg=16)
    whole = D.ref_apply(docs, s)
    for k in (0, 1, 63, 64, 119, 120):
        part = D.ref_apply(docs[k:], dict(s, doc_base=1000 + k))
        first = whole[2].index(k) if k < 120 else len(whole[2])
        assert part[0] == whole[0][first:] and part[1] == whole[1][first:]
        assert [d + k for d in part[2]] == whole[2][first:]
    other = D.ref_apply(docs, dict(s, seed=22))
    assert other[0] != whole[0] and [len(x) for x in other[0]] == [len(x) for x in whole[0]]
    wrap = D.ref_apply(docs[:3], dict(s, doc_base=D.M64))        # the document number wraps
    assert wrap[0][len([d for d in wrap[2] if d == 0]):] == D.ref_apply(docs[1:3], dict(s, doc_base=0))[0]


def test_reference_part_lengths_are_stratified():
    s = D.spec(D.threshold(0.15), 768, seed=1)
    lens = []
    for d in range(200):
        inp, tg = D.ref_unit(s, d, 0, list(range(568)))
        cuts = [i for i, x in enumerate(tg) if x > 30000] + [len(tg)]
        lens += [b - a - 1 for a, b in zip(cuts, cuts[1:])]
    print("noise parts: min %d max %d mean %.3f" % (min(lens), max(lens), sum(lens) / len(lens)))
    # 85 tokens in 28 parts: strata of 2 or 3 excess tokens, so a part has 1 .. 2 * 3 + 1 tokens
    assert min(lens) == 1 and max(lens) <= 7 and abs(sum(lens) / len(lens) - 85 / 28) < 1e-9
    assert len(set(lens)) >= 5
