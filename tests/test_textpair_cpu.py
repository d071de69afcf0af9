"""CPU tests of text pairs (mbpe_textpair_plan, mbpe_textpair_tokens, mbpe_encoder_set_textpair,
mbpe_tok_set_encode_textpair): the symbols are declared, listed and typed and the struct matches the header; every
argument error has its code before any device call; the host's plan equals the reference below -- a literal statement
of the rule, with the removal LOOP for longest_first -- over a grid.  tests/test_gpu_textpair.py uses the same
reference."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import mbpe
from conftest import ROOT

NONE = mbpe.NO_TOKEN
TRUNCATIONS = ("longest_first", "only_first", "only_second")


def ref_keep(truncation, K, la, lb):
    """(a, b) kept of la and lb tokens with room for K (None: no truncation)."""
    a, b = la, lb
    if K is None:
        return a, b
    if truncation == "longest_first":
        while a + b > K:
            if a > b:
                a -= 1
            else:
                b -= 1
    elif truncation == "only_first":
        b = min(lb, K)
        a = min(la, K - b)
    else:
        a = min(la, K)
        b = min(lb, K - a)
    return a, b


def ref_join(A, B, max_tokens=0, truncation="longest_first", sep_ids=(), end_id=None, labels="all", keep_tail_a=False,
             keep_tail_b=False):
    """One pair of token lists -> (joined ids, targets, (a, b)); the keywords are those of mbpe.textpair_spec."""
    end = [] if end_id is None else [end_id]
    K = max_tokens - len(sep_ids) - len(end) if max_tokens else None
    a, b = ref_keep(truncation, K, len(A), len(B))
    ka = A[len(A) - a:] if keep_tail_a else A[:a]
    kb = B[len(B) - b:] if keep_tail_b else B[:b]
    ids = ka + list(sep_ids) + kb + end
    first_b = a + len(sep_ids)
    tgt = [ids[k + 1] if k + 1 < len(ids) and (labels == "all" or k + 1 >= first_b) else NONE for k in range(len(ids))]
    return ids, tgt, (a, b)


def ref_join_all(docs, **kw):
    """Documents 2i and 2i + 1 joined -> (flat ids, flat targets, offsets, kept)."""
    flat, tgt, off, kept = [], [], [0], []
    for i in range(0, len(docs), 2):
        ids, t, ab = ref_join([x & 0x7FFFFFFF for x in docs[i]], [x & 0x7FFFFFFF for x in docs[i + 1]], **kw)
        flat += ids
        tgt += t
        off.append(len(flat))
        kept.append(list(ab))
    return flat, tgt, off, kept


def test_symbols_and_the_struct_match_the_headers():
    L = mbpe.lib()
    header = open(os.path.join(ROOT, "include", "mbpe.h")).read()
    tok_header = open(os.path.join(ROOT, "include", "mbpe_tokenizer.h")).read()
    declared = set(re.findall(r"MBPE_API[^;]*?\b(mbpe_\w+)\s*\(", header + tok_header))
    for s in ("mbpe_textpair_plan", "mbpe_textpair_tokens", "mbpe_textpair_kernel_ms", "mbpe_encoder_set_textpair",
              "mbpe_encoder_textpair_info"):
        assert s in declared and s in mbpe.EXPORTS and getattr(L, s).argtypes, s
    for s in ("mbpe_tok_set_encode_textpair", "mbpe_tok_encode_textpair_info"):
        assert s in declared and s in mbpe.TOK_EXPORTS and getattr(L, s).argtypes, s
    assert L.mbpe_textpair_tokens.argtypes[:8] == L.mbpe_fim_tokens.argtypes[:8] and len(L.mbpe_textpair_tokens.argtypes) == 15
    assert L.mbpe_encoder_textpair_info.argtypes == L.mbpe_tok_encode_textpair_info.argtypes
    for name in ("TextpairSpec", "textpair_spec", "textpair_plan", "textpair_tokens", "textpair_kernel_ms"):
        assert hasattr(mbpe, name), name
    assert hasattr(mbpe.Encoder, "set_textpair") and hasattr(mbpe.Encoder, "textpair_info")
    assert hasattr(mbpe.Tokenizer, "textpair_info")
    for m in ("encode_batch_padded", "encode_batch_aux", "encode_batch_windows", "encode_batch_fit"):
        params = inspect.signature(getattr(mbpe.Tokenizer, m)).parameters
        assert list(params)[-1] == "textpair" and params["textpair"].default is None, m
    body = re.search(r"typedef struct \{([^}]*)\} mbpe_textpair_spec;", header).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"uint32_t\s+(\w+)(?:\[(\d)\])?;", body)
    want = [(n, ctypes.c_uint32 * int(k) if k else ctypes.c_uint32) for n, k in fields]
    assert [(n, ctypes.sizeof(t)) for n, t in want] == [(n, ctypes.sizeof(t)) for n, t in mbpe.TextpairSpec._fields_]
    assert ctypes.sizeof(mbpe.TextpairSpec) == 36 and mbpe.TextpairSpec.end_id.offset == 28
    sp = mbpe.textpair_spec(9, "only_second", sep_ids=(5, 6), end_id=7, labels="second", keep_tail_a=True)
    assert (sp.max_tokens, sp.truncation, sp.keep_tail_a, sp.keep_tail_b, sp.n_sep, list(sp.sep_id), sp.end_id,
            sp.label_mode) == (9, 2, 1, 0, 2, [5, 6], 7, 1)
    assert mbpe.textpair_spec().end_id == NONE


def _spec(**kw):
    sp = mbpe.textpair_spec(sep_ids=(1,), end_id=2)
    for k, v in kw.items():
        if k == "sep0":
            sp.sep_id[0] = v
        else:
            setattr(sp, k, v)
    return sp


ERRORS = [
    ("null spec", None, 32, [0, 3, 10], mbpe.ERR_ARG),
    ("truncation", _spec(truncation=3), 32, [0, 3, 10], mbpe.ERR_ARG),
    ("label_mode", _spec(label_mode=2), 32, [0, 3, 10], mbpe.ERR_ARG),
    ("keep_tail_a", _spec(keep_tail_a=2), 32, [0, 3, 10], mbpe.ERR_ARG),
    ("keep_tail_b", _spec(keep_tail_b=2), 32, [0, 3, 10], mbpe.ERR_ARG),
    ("n_sep", _spec(n_sep=3), 32, [0, 3, 10], mbpe.ERR_ARG),
    ("max_tokens below the constants", _spec(max_tokens=1), 32, [0, 3, 10], mbpe.ERR_ARG),
    ("sep id", _spec(sep0=0x7FFFFFFE), 32, [0, 3, 10], mbpe.ERR_ARG),
    ("end id", _spec(end_id=0x7FFFFFFE), 16, [0, 3, 10], mbpe.ERR_ARG),
    ("odd document count", _spec(), 32, [0, 3, 3, 10], mbpe.ERR_ARG),
    ("descending offsets", _spec(), 32, [0, 5, 3, 3, 10], mbpe.ERR_ARG),
    ("offsets short of the tokens", _spec(), 32, [0, 3, 9], mbpe.ERR_ARG),
    ("token_bits", _spec(), 8, [0, 3, 10], mbpe.ERR_ARG),
    ("sep id in 16 bits", _spec(sep0=65536), 16, [0, 3, 10], mbpe.ERR_VOCAB),
    ("end id in 16 bits", _spec(end_id=0x7FFFFFFD), 16, [0, 3, 10], mbpe.ERR_VOCAB),
]


@pytest.mark.parametrize("what,spec,bits,off,want", ERRORS, ids=[e[0] for e in ERRORS])
def test_argument_errors_come_before_the_device(what, spec, bits, off, want):
    L = mbpe.lib()
    tokens = np.arange(10, dtype=np.uint16 if bits == 16 else np.uint32)
    o = np.array(off, dtype=np.uint64)
    out, tgt = np.full(64, 0xAB, dtype=np.uint8), np.full(16, 77, dtype=np.uint32)
    new_off, kept, n = np.full(4, 77, dtype=np.uint64), np.full(8, 77, dtype=np.uint64), ctypes.c_uint64(77)
    rc = L.mbpe_textpair_tokens(0, tokens.ctypes.data, 10, bits, 0, o.ctypes.data, len(o) - 1,
                                ctypes.byref(spec) if spec else None, out.ctypes.data, tgt.ctypes.data, 16, 0,
                                new_off.ctypes.data, kept.ctypes.data, ctypes.byref(n))
    assert (rc, n.value) == (want, 0) and L.mbpe_last_error()
    assert (out == 0xAB).all() and (tgt == 77).all() and (new_off == 77).all() and (kept == 77).all()
    if bits == 32 and off[-1] == 10:                             # the plan alone (it has no token count) refuses the same
        assert L.mbpe_textpair_plan(o.ctypes.data, len(o) - 1, ctypes.byref(spec) if spec else None, new_off.ctypes.data,
                                    kept.ctypes.data) == want
        assert (new_off == 77).all() and (kept == 77).all()


def test_handles_and_the_query():
    L = mbpe.lib()
    ok, n = _spec(), ctypes.c_uint64(77)
    assert L.mbpe_encoder_set_textpair(None, ctypes.byref(ok)) == mbpe.ERR_ARG
    assert L.mbpe_encoder_textpair_info(None, None, 0, ctypes.byref(n)) == mbpe.ERR_ARG
    assert L.mbpe_tok_set_encode_textpair(None, ctypes.byref(ok)) == mbpe.ERR_ARG
    assert L.mbpe_textpair_kernel_ms(None) == mbpe.ERR_ARG
    tok = mbpe.Tokenizer("")
    assert L.mbpe_tok_set_encode_textpair(tok._h, ctypes.byref(_spec(n_sep=3))) == mbpe.ERR_ARG
    assert L.mbpe_tok_set_encode_textpair(tok._h, ctypes.byref(ok)) == mbpe.OK
    assert L.mbpe_tok_set_encode_textpair(tok._h, None) == mbpe.OK
    assert tok.textpair_info().shape == (0, 2)
    tok.close()
    # tokens_out NULL is a query, answered without a device; a cap too small still reports the count
    tokens, o = np.arange(10, dtype=np.uint32), np.array([0, 3, 10], dtype=np.uint64)
    new_off, out = np.zeros(2, dtype=np.uint64), np.full(16, 77, dtype=np.uint32)
    head = (0, tokens.ctypes.data, 10, 32, 0, o.ctypes.data, 2, ctypes.byref(_spec(max_tokens=8)))
    assert L.mbpe_textpair_tokens(*head, None, None, 0, 0, new_off.ctypes.data, None, ctypes.byref(n)) == mbpe.OK
    assert n.value == 8 and new_off.tolist() == [0, 8]
    assert L.mbpe_textpair_tokens(*head, out.ctypes.data, None, 7, 0, None, None, ctypes.byref(n)) == mbpe.ERR_ARG
    assert n.value == 8 and (out == 77).all() and b"too small" in L.mbpe_last_error()


@pytest.mark.parametrize("K", list(range(10)) + [None])
@pytest.mark.parametrize("truncation", TRUNCATIONS)
def test_plan_equals_the_reference(truncation, K):
    lens = [(la, lb) for la in range(12) for lb in range(12)]
    off = np.concatenate([[0], np.cumsum([x for p in lens for x in p])]).astype(np.uint64)
    spec = mbpe.textpair_spec(0 if K is None else K + 2, truncation, sep_ids=(1,), end_id=2)
    want = [ref_keep(truncation, K, la, lb) for la, lb in lens]
    new_off, kept = mbpe.textpair_plan(off, spec)
    assert kept.tolist() == [list(w) for w in want]
    assert new_off.tolist() == [0] + np.cumsum([a + b + 2 for a, b in want]).tolist()
