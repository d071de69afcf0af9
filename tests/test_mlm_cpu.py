"""CPU tests of masked-LM batches (mbpe_mlm_plan, mbpe_mlm_tokens, the _labels pack calls, mbpe_encoder_set_mlm,
mbpe_tok_set_encode_mlm): the symbols exist, are listed and typed and the struct matches the header; every argument
error has its code before any device call and writes nothing; the host's plan equals the rule restated in Python
(mlm_cases.ref_apply) over a grid; csrc/mlm.h passes its stand-alone check (tests/mlm_check.cpp), plain and under ASan +
UBSan, and gives the reference's answers there too; the draws are spread as a binomial is; and the reference has the
properties the rule promises."""
import ctypes
import inspect
import os
import random
import re
import subprocess

import numpy as np
import pytest

import mbpe
from conftest import ROOT
import mlm_cases as M

HERE = os.path.dirname(os.path.abspath(__file__))
NEW = ("mbpe_mlm_plan", "mbpe_mlm_tokens", "mbpe_mlm_kernel_ms", "mbpe_pack_tokens_aux_labels", "mbpe_pack_windows_labels",
       "mbpe_pack_fit_labels", "mbpe_encoder_set_mlm")
NEW_TOK = ("mbpe_tok_set_encode_mlm",)
FILL = 0xAB


def _has_gpu():
    import torch
    return torch.cuda.is_available()


def _c(s):
    """mlm_cases.spec -> mbpe.MlmSpec"""
    p = list(s["protect"])
    return mbpe.MlmSpec(s["select"], s["mask"], s["random"], s["seed"], s["doc_base"], s["mask_id"], s["vocab_n"],
                        s["whole_word"], len(p), (ctypes.c_uint32 * 8)(*p[:8]))


def test_exports_and_the_mlm_struct_match_the_headers():
    L = mbpe.lib()
    header = open(os.path.join(ROOT, "include", "mbpe.h")).read()
    declared = set(re.findall(r"MBPE_API[^;]*?\b(mbpe_\w+)\s*\(", header))
    tok_header = open(os.path.join(ROOT, "include", "mbpe_tokenizer.h")).read()
    tok_declared = set(re.findall(r"MBPE_API[^;]*?\b(mbpe_tok_\w+)\s*\(", tok_header))
    for s in NEW:
        assert s in declared and s in mbpe.EXPORTS and hasattr(L, s) and getattr(L, s).argtypes, s
    for s in NEW_TOK:
        assert s in tok_declared and s in mbpe.TOK_EXPORTS and hasattr(L, s) and getattr(L, s).argtypes, s
    # mbpe_mlm_tokens has the conventions of mbpe_fim_tokens up to the spec; each _labels call is its call plus one pointer
    assert L.mbpe_mlm_tokens.argtypes[:8] == L.mbpe_fim_tokens.argtypes[:8]
    assert len(L.mbpe_mlm_tokens.argtypes) == 11 and len(L.mbpe_mlm_plan.argtypes) == 8
    for name in ("mbpe_pack_tokens_aux", "mbpe_pack_windows", "mbpe_pack_fit"):
        assert getattr(L, name + "_labels").argtypes == getattr(L, name).argtypes + [ctypes.c_void_p], name
    assert L.mbpe_encoder_set_mlm.argtypes == L.mbpe_tok_set_encode_mlm.argtypes == [ctypes.c_void_p] * 2
    for name in ("MlmSpec", "mlm_spec", "mlm_plan", "mlm_tokens", "mlm_kernel_ms"):
        assert hasattr(mbpe, name), name
    assert hasattr(mbpe.Encoder, "set_mlm")
    for m in ("encode_batch_aux", "encode_batch_windows", "encode_batch_fit"):
        assert inspect.signature(getattr(mbpe.Tokenizer, m)).parameters["mlm"].default is None, m
    for f in (mbpe.pack_tokens_aux, mbpe.pack_windows, mbpe.pack_fit):
        assert inspect.signature(f).parameters["label_tokens"].default is None, f
    body = re.search(r"typedef struct \{([^}]*)\} mbpe_mlm_spec;", header).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for typ, names in re.findall(r"(uint\d+_t)\s+([^;]+);", body):
        fields += [(n.strip(), typ) for n in names.split(",")]
    ctype = {"uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32}
    got = [(n, ctype[t]) if "[" not in n else (n.split("[")[0], ctype[t] * int(n.split("[")[1].rstrip("]")))
           for n, t in fields]
    want = list(mbpe.MlmSpec._fields_)
    assert [n for n, _ in got] == [n for n, _ in want] == ["select", "mask", "random", "seed", "doc_base", "mask_id",
                                                            "vocab_n", "whole_word", "n_protect", "protect"]
    assert all(ctypes.sizeof(a[1]) == ctypes.sizeof(b[1]) for a, b in zip(got, want))
    assert ctypes.sizeof(mbpe.MlmSpec) == 88 and mbpe.MlmSpec.mask_id.offset == 40 and mbpe.MlmSpec.protect.offset == 56
    sp = mbpe.mlm_spec(0.5, 7, 9, mask_share=1.0, random_share=0.0, seed=-1, doc_base=1 << 40, whole_word=True, protect=(3, 4))
    assert (sp.select, sp.mask, sp.random, sp.seed, sp.doc_base) == (1 << 31, 1 << 32, 0, (1 << 64) - 1, 1 << 40)
    assert (sp.mask_id, sp.vocab_n, sp.whole_word, sp.n_protect, list(sp.protect)[:3]) == (7, 9, 1, 2, [3, 4, 0])
    sp = mbpe.mlm_spec(0.15, 7, 9)
    assert (sp.select, sp.mask, sp.random) == (M.threshold(0.15), M.threshold(0.8), M.threshold(0.1))
    with pytest.raises(mbpe.MbpeError):
        mbpe.mlm_spec(1.5, 1, 2)
    with pytest.raises(mbpe.MbpeError):
        mbpe.mlm_spec(0.5, 1, 2, protect=range(9))


# ---- argument errors before the device ------------------------------------------------------------------------------------

T16 = np.arange(10, dtype=np.uint16)
T32 = np.arange(10, dtype=np.uint32)
OFF = [0, 3, 3, 10]


def _tokens(tokens, off, spec, on_device=0, shift=0, tshift=0, spec_null=False, out_null=False, bits=None):
    """mbpe_mlm_tokens as it is, into prefilled host buffers (with on_device=1 the same buffers are named as device
    memory: such a call must be refused before anything is done with them) -> (code, the buffers)."""
    t = np.ascontiguousarray(tokens)
    o = np.ascontiguousarray(off, dtype=np.uint64)
    bufs = [np.full(1024, FILL, dtype=np.uint8), np.full(1024, FILL, dtype=np.uint8)]       # tokens, targets
    base = [b.ctypes.data + (-b.ctypes.data) % 16 for b in bufs]
    rc = mbpe.lib().mbpe_mlm_tokens(
        0, t.ctypes.data if len(t) else None, len(t), bits or t.dtype.itemsize * 8, 0, o.ctypes.data, len(o) - 1,
        None if spec_null else ctypes.byref(spec), None if out_null else base[0] + shift, base[1] + tshift, on_device)
    return rc, bufs


def _untouched(bufs):
    return all((b.view(np.uint8) == FILL).all() for b in bufs)


def _plan(tokens, off, spec, bits=None, spec_null=False):
    t = np.ascontiguousarray(tokens)
    o = np.ascontiguousarray(off, dtype=np.uint64)
    bufs = [np.full(256, FILL, dtype=np.uint8), np.full(256, FILL, dtype=np.uint8)]
    rc = mbpe.lib().mbpe_mlm_plan(t.ctypes.data, len(t), bits or t.dtype.itemsize * 8, o.ctypes.data, len(o) - 1,
                                  None if spec_null else ctypes.byref(spec), bufs[0].ctypes.data, bufs[1].ctypes.data)
    return rc, bufs


ERRORS = [
    (dict(spec_null=True), M.spec(), T32, mbpe.ERR_ARG),
    (dict(bits=8), M.spec(), T32, mbpe.ERR_ARG),
    ({}, M.spec(select=M.ONE + 1), T32, mbpe.ERR_ARG),
    ({}, M.spec(mask=M.ONE + 1, random=0), T32, mbpe.ERR_ARG),
    ({}, M.spec(mask=0, random=M.ONE + 1), T32, mbpe.ERR_ARG),
    ({}, M.spec(mask=M.ONE // 2, random=M.ONE // 2 + 1), T32, mbpe.ERR_ARG),
    ({}, M.spec(vocab_n=0), T32, mbpe.ERR_ARG),
    ({}, M.spec(whole_word=2), T32, mbpe.ERR_ARG),
    ({}, M.spec(mask_id=0x7FFFFFFE), T32, mbpe.ERR_ARG),
    ({}, M.spec(mask_id=0xFFFFFFFF), T16, mbpe.ERR_ARG),
    ({}, M.spec(vocab_n=0x7FFFFFFE), T32, mbpe.ERR_ARG),
    ({}, M.spec(whole_word=1), T16, mbpe.ERR_ARG),
    ({}, M.spec(mask_id=65536), T16, mbpe.ERR_VOCAB),
    ({}, M.spec(mask_id=5, vocab_n=65537), T16, mbpe.ERR_VOCAB),
]


def test_mlm_argument_errors_come_before_the_device():
    L = mbpe.lib()
    nine = _c(M.spec())
    nine.n_protect = 9
    cases = [(kw, _c(s), t, want) for kw, s, t, want in ERRORS] + [({}, nine, T32, mbpe.ERR_ARG)]
    for kw, spec, tokens, want in cases:
        rc, bufs = _tokens(tokens, OFF, spec, **kw)
        assert rc == want, (kw, list(bytes(spec)), rc)
        assert _untouched(bufs), kw
        assert L.mbpe_last_error()
        rc, bufs = _plan(tokens, OFF, spec, **kw)                # the host's plan has the same rules
        assert rc == want and _untouched(bufs), kw
    ok = _c(M.spec(mask_id=5, vocab_n=100))
    for kw, tokens in ((dict(out_null=True), T32), (dict(on_device=1, shift=2), T32), (dict(on_device=1, shift=1), T16),
                       (dict(on_device=1, tshift=2), T16)):
        rc, bufs = _tokens(tokens, OFF, ok, **kw)
        assert rc == mbpe.ERR_ARG and _untouched(bufs), kw
    # bad offsets: descending, not from 0, not to n_tokens
    for bad in ([0, 5, 3, 10], [1, 3, 3, 10], [0, 3, 3, 9]):
        rc, bufs = _tokens(T32, bad, ok)
        assert rc == mbpe.ERR_ARG and _untouched(bufs)
        rc, bufs = _plan(T32, bad, ok)
        assert rc == mbpe.ERR_ARG and _untouched(bufs)
    assert L.mbpe_mlm_plan(None, 10, 32, np.array(OFF, dtype=np.uint64).ctypes.data, 3, ctypes.byref(ok), None, None) == mbpe.ERR_ARG
    # nothing to do is no device call
    rc, bufs = _tokens(np.zeros(0, dtype=np.uint32), [0, 0, 0], ok)
    assert rc == mbpe.OK and _untouched(bufs)
    got, tgt = mbpe.mlm_tokens(np.zeros(0, dtype=np.uint16), [0], ok)
    assert got.shape == tgt.shape == (0,) and got.dtype == np.uint16 and tgt.dtype == np.uint32
    ms = ctypes.c_float(5)
    assert L.mbpe_mlm_kernel_ms(None) == mbpe.ERR_ARG and L.mbpe_mlm_kernel_ms(ctypes.byref(ms)) == mbpe.OK
    # the encoder's and the tokenizer's entry points
    assert L.mbpe_encoder_set_mlm(None, ctypes.byref(ok)) == mbpe.ERR_ARG
    assert L.mbpe_tok_set_encode_mlm(None, ctypes.byref(ok)) == mbpe.ERR_ARG
    tok = mbpe.Tokenizer("")
    assert L.mbpe_tok_set_encode_mlm(tok._h, ctypes.byref(_c(M.spec(select=M.ONE + 1)))) == mbpe.ERR_ARG
    assert L.mbpe_tok_set_encode_mlm(tok._h, ctypes.byref(_c(M.spec(mask_id=0x7FFFFFFE)))) == mbpe.ERR_ARG
    assert L.mbpe_tok_set_encode_mlm(tok._h, ctypes.byref(_c(M.spec(whole_word=1)))) == mbpe.OK
    assert L.mbpe_tok_set_encode_mlm(tok._h, None) == mbpe.OK
    tok.close()


def test_label_calls_refuse_a_missing_target_stream_before_the_device():
    L = mbpe.lib()
    spec = mbpe.pack_spec(8, "packed")
    aux = mbpe.PackAux(None, None, None, -100)
    off = np.array(OFF, dtype=np.uint64)
    n = ctypes.c_uint64(77)
    head = (0, T32.ctypes.data, 10, 32, 0, off.ctypes.data, 3, ctypes.byref(spec), None, 0, 0, None, ctypes.byref(n),
            ctypes.byref(aux))
    win, fit = mbpe.PackWindow(0, 0, None, None), mbpe.PackFit(None, None)
    pad = mbpe.pack_spec(8, "padded")
    head_pad = head[:7] + (ctypes.byref(pad),) + head[8:]
    assert L.mbpe_pack_tokens_aux_labels(*head, None) == mbpe.ERR_ARG and n.value == 0
    assert L.mbpe_pack_windows_labels(*head_pad, ctypes.byref(win), None) == mbpe.ERR_ARG
    assert L.mbpe_pack_fit_labels(*head, ctypes.byref(fit), None) == mbpe.ERR_ARG
    assert b"_labels" in L.mbpe_last_error()
    # with one, the query is answered on the host as it is without
    lab = np.zeros(10, dtype=np.uint32)
    assert L.mbpe_pack_tokens_aux_labels(*head, lab.ctypes.data) == mbpe.OK and n.value == 2
    assert L.mbpe_pack_windows_labels(*head_pad, ctypes.byref(win), lab.ctypes.data) == mbpe.OK and n.value == 3
    assert L.mbpe_pack_fit_labels(*head, ctypes.byref(fit), lab.ctypes.data) == mbpe.OK and n.value == 2
    with pytest.raises(ValueError):
        mbpe.pack_tokens_aux(T32, OFF, 8, label_tokens=lab[:9])


# ---- the plan against the reference ----------------------------------------------------------------------------------------

def _grid():
    rng = random.Random(3)
    for lens in ([], [0], [1], [0, 1, 2, 0, 5], M.split_lens(300, rng, 9), [1030], M.split_lens(2049, rng, 40)):
        ids, ends, off = M.stream(lens, rng, hi=60000)
        for select in (0.0, 0.15, 0.5, 1.0):
            for ww in (0, 1):
                for base in (0, (1 << 64) - 3):
                    yield ids, ends, off, M.spec(M.threshold(select), seed=len(lens) + 7, doc_base=base, whole_word=ww,
                                                 protect=tuple(ids[:2]))


def test_plan_equals_the_reference_over_the_grid():
    n_cases = 0
    for ids, ends, off, s in _grid():
        want_out, want_tgt = M.ref_apply(s, ids, ends, off)
        out, tgt = mbpe.mlm_plan(M.flagged(ids, ends), off, _c(s))
        assert out.dtype == np.uint32 and out.tolist() == want_out and tgt.tolist() == want_tgt, (len(ids), s)
        if not s["whole_word"]:                                  # 16-bit tokens; the ends play no part
            out, tgt = mbpe.mlm_plan(np.array(ids, dtype=np.uint16), off, _c(s))
            assert out.dtype == np.uint16 and out.tolist() == want_out and tgt.tolist() == want_tgt
            out, tgt = mbpe.mlm_plan(np.array(ids, dtype=np.uint32), off, _c(s))
            assert out.tolist() == want_out and tgt.tolist() == want_tgt
        else:                                                    # word_ends= is bit 31
            out2, tgt2 = mbpe.mlm_plan(np.array(ids, dtype=np.uint32), off, _c(s), word_ends=ends)
            assert out2.tolist() == want_out and tgt2.tolist() == want_tgt
        n_cases += 1
    assert n_cases == 7 * 4 * 2 * 2
    for p in (0.0, 0.15, 0.8, 1.0):
        assert mbpe.dropout_threshold(p) == M.threshold(p)


@pytest.mark.skipif(_has_gpu(), reason="checks the no-device failure path")
def test_no_cpu_fallback():
    ok = _c(M.spec(mask_id=5, vocab_n=100))
    rc, bufs = _tokens(T32, OFF, ok)
    assert rc == mbpe.ERR_NO_DEVICE and _untouched(bufs)
    with pytest.raises(mbpe.MbpeError) as e:
        mbpe.mlm_tokens(T16, OFF, _c(M.spec(select=0, mask_id=5)))
    assert e.value.code == mbpe.ERR_NO_DEVICE
    with pytest.raises(mbpe.MbpeError) as e:
        mbpe.pack_tokens_aux(T32, OFF, 8, labels=True, label_tokens=np.zeros(10, dtype=np.uint32))
    assert e.value.code == mbpe.ERR_NO_DEVICE
    tok = mbpe.Tokenizer("")
    tok.set_merges(np.array([[97, 98]], dtype=np.uint32))
    with pytest.raises(mbpe.MbpeError) as e:
        tok.encode_batch_aux([b"abab", b"", b"ab"], 8, labels=True, mlm=mbpe.mlm_spec(0.5, 300, 256))
    assert e.value.code == mbpe.ERR_NO_DEVICE
    tok.close()


# ---- mlm.h as a stand-alone program ---------------------------------------------------------------------------------------

FLAGS = {
    "plain": ["-O2"],
    "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
}


@pytest.mark.parametrize("build", sorted(FLAGS))
def test_mlm_rule(build, tmp_path):
    exe = str(tmp_path / "mlm_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Wextra", "-Werror"] + FLAGS[build] +
                          ["-I" + os.path.join(ROOT, "minbpe-cc_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                           os.path.join(HERE, "mlm_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert re.search(r"ok: \d+ checks, 0 failures\s*$", r.stdout)
    # the header's host loop over the grid's cases gives the reference's answers
    cases = [c for c in _grid() if len(c[0])]
    lines = [str(2 * len(cases))]
    want = []
    for ids, ends, off, s in cases:
        for bits in (32, 16):
            s2 = dict(s, whole_word=s["whole_word"] if bits == 32 else 0, mask_id=50001 if bits == 32 else 40001)
            p = list(s2["protect"]) + [0] * (8 - len(s2["protect"]))
            toks = M.flagged(ids, ends).tolist() if bits == 32 else ids
            lines.append(" ".join(map(str, [s2["select"], s2["mask"], s2["random"], s2["seed"], s2["doc_base"], s2["mask_id"],
                                            s2["vocab_n"], s2["whole_word"], len(s2["protect"])] + p +
                                      [bits, len(off) - 1, len(ids)] + off.tolist() + toks)))
            want += list(M.ref_apply(s2, ids, ends, off))
    r = subprocess.run([exe, "apply"], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = [[int(x) for x in line.split()] for line in r.stdout.split("\n")[:-1]]
    assert len(got) == len(want) == 4 * len(cases)
    assert got == want


# ---- the reference is the specification: its own invariants ---------------------------------------------------------------

@pytest.mark.parametrize("seed", [0, 1, 12345])
def test_reference_draws_are_spread(seed):
    # 100 documents of 1,000 tokens, rate 0.15, shares 0.8 / 0.1: 6 sigma of the binomial around the expectation
    rng = random.Random(1)
    ids, ends, off = M.stream([1000] * 100, rng)
    s = M.spec(seed=seed)
    out, tgt = M.ref_apply(s, ids, ends, off)
    sel = [i for i, t in enumerate(tgt) if t != M.NO_TOKEN]
    masked = sum(out[i] == M.MASK_ID for i in sel)
    r = [M.ref_hash(M.doc_seed(s, i // 1000), i % 1000, 1) for i in sel]
    rand = sum(s["mask"] <= x < s["mask"] + s["random"] for x in r)
    print("seed %d: selected %d, mask_id %d, random %d" % (seed, len(sel), masked, rand))
    assert abs(len(sel) - 15000) <= 678
    assert abs(masked - 12000) <= 294
    assert abs(rand - 1500) <= 220
    assert masked == sum(x < s["mask"] for x in r)
    assert len(sel) == {0: 15016, 1: 15005, 12345: 15008}[seed]   # the figures the thresholds were checked with


def test_reference_composes_over_batches_and_layouts():
    rng = random.Random(5)
    lens = [rng.randrange(0, 30) for _ in range(200)]
    ids, ends, off = M.stream(lens, rng)
    for ww in (0, 1):
        s = M.spec(M.threshold(0.5), seed=21, doc_base=1000, whole_word=ww)
        whole = M.ref_apply(s, ids, ends, off)
        for k in (0, 1, 63, 64, 199, 200):
            a = int(off[k])
            part = M.ref_apply(dict(s, doc_base=1000 + k), ids[a:], ends[a:], off[k:] - off[k])
            assert part == (whole[0][a:], whole[1][a:])
        assert M.ref_apply(dict(s, seed=22), ids, ends, off) != whole


def test_reference_properties():
    rng = random.Random(9)
    ids, ends, off = M.stream(M.split_lens(3000, rng, 30), rng, hi=1000)
    prot = (ids[0], ids[5], ids[17])
    # within a word, all unprotected tokens are targets or none is
    s = M.spec(M.threshold(0.3), seed=4, whole_word=1, protect=prot)
    out, tgt = M.ref_apply(s, ids, ends, off)
    n_words = n_hit = 0
    for d in range(len(off) - 1):
        a, b = int(off[d]), int(off[d + 1])
        w0 = a
        for i in range(a, b):
            if ends[i] or i == b - 1:
                hits = {tgt[j] != M.NO_TOKEN for j in range(w0, i + 1) if ids[j] not in prot}
                assert len(hits) <= 1
                assert all(tgt[j] == M.NO_TOKEN and out[j] == ids[j] for j in range(w0, i + 1) if ids[j] in prot)
                n_words += 1
                n_hit += hits == {True}
                w0 = i + 1
    assert 0.2 < n_hit / n_words < 0.4
    for ww in (0, 1):
        # select 0: the identity with no targets; select 2^32: every unprotected token a target
        out, tgt = M.ref_apply(M.spec(0, whole_word=ww, protect=prot), ids, ends, off)
        assert out == ids and set(tgt) == {M.NO_TOKEN}
        out, tgt = M.ref_apply(M.spec(M.ONE, whole_word=ww, protect=prot), ids, ends, off)
        assert all((t == M.NO_TOKEN) == (i in prot) and (t == i or i in prot) for i, t in zip(ids, tgt))
        # mask 2^32: all mask_id; random 2^32: all below vocab_n; both 0: the ids stay, the targets are set
        out, tgt = M.ref_apply(M.spec(M.ONE, M.ONE, 0, whole_word=ww), ids, ends, off)
        assert set(out) == {M.MASK_ID} and tgt == ids
        out, tgt = M.ref_apply(M.spec(M.ONE, 0, M.ONE, vocab_n=7, whole_word=ww), ids, ends, off)
        assert set(out) == set(range(7)) and tgt == ids
        out, tgt = M.ref_apply(M.spec(M.ONE, 0, 0, whole_word=ww), ids, ends, off)
        assert out == ids and tgt == ids
