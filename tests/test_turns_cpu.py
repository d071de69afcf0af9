"""CPU tests of multi-turn conversation batches (mbpe_turns_plan, mbpe_turns_tokens, mbpe_encoder_set_turns,
mbpe_tok_set_encode_turns): the symbols are declared, listed and typed and the struct matches the header; every argument
error has its code before any device call and writes nothing; the host's plan equals tests/turns_cases.py over the
three truncations."""
import ctypes
import inspect
import os
import random
import re

import numpy as np
import pytest

import mbpe
import turns_cases as T
from conftest import ROOT


def test_symbols_and_the_struct_match_the_headers():
    L = mbpe.lib()
    header = open(os.path.join(ROOT, "include", "mbpe.h")).read()
    tok_header = open(os.path.join(ROOT, "include", "mbpe_tokenizer.h")).read()
    declared = set(re.findall(r"MBPE_API[^;]*?\b(mbpe_\w+)\s*\(", header + tok_header))
    for s in ("mbpe_turns_plan", "mbpe_turns_tokens", "mbpe_turns_kernel_ms", "mbpe_encoder_set_turns",
              "mbpe_encoder_turns_info"):
        assert s in declared and s in mbpe.EXPORTS and getattr(L, s).argtypes, s
    for s in ("mbpe_tok_set_encode_turns", "mbpe_tok_encode_turns_info"):
        assert s in declared and s in mbpe.TOK_EXPORTS and getattr(L, s).argtypes, s
    assert L.mbpe_turns_tokens.argtypes[:7] == L.mbpe_textpair_tokens.argtypes[:7] and len(L.mbpe_turns_tokens.argtypes) == 18
    assert L.mbpe_encoder_turns_info.argtypes == L.mbpe_tok_encode_turns_info.argtypes
    assert L.mbpe_encoder_set_turns.argtypes == L.mbpe_tok_set_encode_turns.argtypes
    for name in ("TurnsSpec", "turns_spec", "turns_plan", "turns_tokens", "turns_kernel_ms"):
        assert hasattr(mbpe, name), name
    assert hasattr(mbpe.Encoder, "set_turns") and hasattr(mbpe.Encoder, "turns_info") and hasattr(mbpe.Tokenizer, "turns_info")
    for m in ("encode_batch_padded", "encode_batch_aux", "encode_batch_windows", "encode_batch_fit"):
        params = inspect.signature(getattr(mbpe.Tokenizer, m)).parameters
        assert list(params)[-2:] == ["turns", "textpair"] and params["turns"].default is None, m
    body = re.search(r"typedef struct \{([^}]*)\} mbpe_turns_spec;", header).group(1)
    fields = re.findall(r"uint32_t\s+(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [n for n, _ in mbpe.TurnsSpec._fields_] and all(t is ctypes.c_uint32 for _, t in mbpe.TurnsSpec._fields_)
    assert ctypes.sizeof(mbpe.TurnsSpec) == 24
    for name, py in (("TURN_TRAIN", mbpe.TURN_TRAIN), ("TURN_NO_END", mbpe.TURN_NO_END), ("TURNS_RIGHT", mbpe.TURNS_RIGHT),
                     ("TURNS_LEFT", mbpe.TURNS_LEFT), ("TURNS_DROP_OLDEST", mbpe.TURNS_DROP_OLDEST),
                     ("TURNS_LABEL_ALL", mbpe.TURNS_LABEL_ALL), ("TURNS_LABEL_TRAINED", mbpe.TURNS_LABEL_TRAINED)):
        assert int(re.search(r"#define MBPE_%s\s+(\d+)u" % name, header).group(1)) == py, name
    sp = mbpe.turns_spec(9, "drop_oldest", head_turns=1, turn_end_id=5, end_id=7, labels="all")
    assert (sp.max_tokens, sp.truncation, sp.head_turns, sp.turn_end_id, sp.end_id, sp.label_mode) == (9, 2, 1, 5, 7, 0)
    sp = mbpe.turns_spec()
    assert (sp.turn_end_id, sp.end_id, sp.label_mode) == (T.NONE, T.NONE, 1)


def _spec(**kw):
    sp = mbpe.turns_spec(turn_end_id=1, end_id=2)
    for k, v in kw.items():
        setattr(sp, k, v)
    return sp


# (name, spec, token bits, token offsets, turn_off, flags, code): 10 tokens in three turns
ERRORS = [
    ("null spec", None, 32, [0, 3, 3, 10], [0, 2, 3], [1, 0, 2], mbpe.ERR_ARG),
    ("truncation", _spec(truncation=3), 32, [0, 3, 3, 10], [0, 2, 3], [1, 0, 2], mbpe.ERR_ARG),
    ("label_mode", _spec(label_mode=2), 32, [0, 3, 3, 10], [0, 2, 3], [1, 0, 2], mbpe.ERR_ARG),
    ("turn_end_id", _spec(turn_end_id=0x7FFFFFFE), 32, [0, 3, 3, 10], [0, 2, 3], [1, 0, 2], mbpe.ERR_ARG),
    ("end_id", _spec(end_id=0x7FFFFFFE), 16, [0, 3, 3, 10], [0, 2, 3], [1, 0, 2], mbpe.ERR_ARG),
    ("flag bit 2", _spec(), 32, [0, 3, 3, 10], [0, 2, 3], [1, 4, 2], mbpe.ERR_ARG),
    ("null turn_off", _spec(), 32, [0, 3, 3, 10], None, [1, 0, 2], mbpe.ERR_ARG),
    ("null flags", _spec(), 32, [0, 3, 3, 10], [0, 2, 3], None, mbpe.ERR_ARG),
    ("turn_off begins above 0", _spec(), 32, [0, 3, 3, 10], [1, 2, 3], [1, 0, 2], mbpe.ERR_ARG),
    ("turn_off descends", _spec(), 32, [0, 3, 3, 10], [0, 2, 1, 3], [1, 0, 2], mbpe.ERR_ARG),
    ("turn_off ends short", _spec(), 32, [0, 3, 3, 10], [0, 2, 2], [1, 0, 2], mbpe.ERR_ARG),
    ("descending offsets", _spec(), 32, [0, 5, 3, 10], [0, 2, 3], [1, 0, 2], mbpe.ERR_ARG),
    ("offsets short of the tokens", _spec(), 32, [0, 3, 3, 9], [0, 2, 3], [1, 0, 2], mbpe.ERR_ARG),
    ("token_bits", _spec(), 8, [0, 3, 3, 10], [0, 2, 3], [1, 0, 2], mbpe.ERR_ARG),
    ("turn_end_id in 16 bits", _spec(turn_end_id=65536), 16, [0, 3, 3, 10], [0, 2, 3], [1, 0, 2], mbpe.ERR_VOCAB),
    ("end_id in 16 bits", _spec(end_id=0x7FFFFFFD), 16, [0, 3, 3, 10], [0, 2, 3], [1, 0, 2], mbpe.ERR_VOCAB),
]


@pytest.mark.parametrize("what,spec,bits,off,turn_off,flags,want", ERRORS, ids=[e[0] for e in ERRORS])
def test_argument_errors_come_before_the_device(what, spec, bits, off, turn_off, flags, want):
    L = mbpe.lib()
    tokens = np.arange(10, dtype=np.uint16 if bits == 16 else np.uint32)
    o = np.array(off, dtype=np.uint64)
    to = None if turn_off is None else np.array(turn_off, dtype=np.uint64)
    fl = None if flags is None else np.array(flags, dtype=np.uint8)
    n_convs = 2 if to is None else len(to) - 1
    arrays = (o.ctypes.data, len(o) - 1, None if to is None else to.ctypes.data, n_convs, None if fl is None else fl.ctypes.data,
              ctypes.byref(spec) if spec else None)
    out, tgt = np.full(64, 0xAB, dtype=np.uint8), np.full(16, 77, dtype=np.uint32)
    new_off, info, n = np.full(5, 77, dtype=np.uint64), np.full(8, 77, dtype=np.uint64), ctypes.c_uint64(77)
    rc = L.mbpe_turns_tokens(0, tokens.ctypes.data, 10, bits, 0, *arrays, out.ctypes.data, tgt.ctypes.data, 16, 0,
                             new_off.ctypes.data, info.ctypes.data, ctypes.byref(n))
    assert (rc, n.value) == (want, 0) and L.mbpe_last_error()
    assert (out == 0xAB).all() and (tgt == 77).all() and (new_off == 77).all() and (info == 77).all()
    if bits == 32 and off[-1] == 10:                             # the plan alone (it has no token count) refuses the same
        assert L.mbpe_turns_plan(*arrays, new_off.ctypes.data, info.ctypes.data) == want
        assert (new_off == 77).all() and (info == 77).all()
        if spec is not None and "offsets" not in what and "ends short" not in what:
            # and so does the setter, which sees neither token offsets nor a document count
            tok = mbpe.Tokenizer("")
            assert L.mbpe_tok_set_encode_turns(tok._h, *arrays[5:], *arrays[2:5]) == want
            tok.close()


def test_handles_and_the_query():
    L = mbpe.lib()
    ok, n = _spec(), ctypes.c_uint64(77)
    to, fl = np.array([0, 2, 3], dtype=np.uint64), np.array([1, 0, 2], dtype=np.uint8)
    assert L.mbpe_encoder_set_turns(None, ctypes.byref(ok), to.ctypes.data, 2, fl.ctypes.data) == mbpe.ERR_ARG
    assert L.mbpe_encoder_turns_info(None, None, 0, ctypes.byref(n)) == mbpe.ERR_ARG
    assert L.mbpe_tok_set_encode_turns(None, ctypes.byref(ok), to.ctypes.data, 2, fl.ctypes.data) == mbpe.ERR_ARG
    assert L.mbpe_turns_kernel_ms(None) == mbpe.ERR_ARG
    tok = mbpe.Tokenizer("")
    assert L.mbpe_tok_set_encode_turns(tok._h, ctypes.byref(ok), to.ctypes.data, 2, fl.ctypes.data) == mbpe.OK
    assert L.mbpe_tok_set_encode_turns(tok._h, None, None, 0, None) == mbpe.OK
    assert tok.turns_info().shape == (0, 2)
    tok.close()
    # tokens_out NULL is a query, answered without a device; a cap too small still reports the count
    tokens, o = np.arange(10, dtype=np.uint32), np.array([0, 3, 3, 10], dtype=np.uint64)
    new_off, out = np.zeros(3, dtype=np.uint64), np.full(16, 77, dtype=np.uint32)
    head = (0, tokens.ctypes.data, 10, 32, 0, o.ctypes.data, 3, to.ctypes.data, 2, fl.ctypes.data, ctypes.byref(_spec(max_tokens=6)))
    assert L.mbpe_turns_tokens(*head, None, None, 0, 0, new_off.ctypes.data, None, ctypes.byref(n)) == mbpe.OK
    assert n.value == 12 and new_off.tolist() == [0, 6, 12]
    assert L.mbpe_turns_tokens(*head, out.ctypes.data, None, 11, 0, None, None, ctypes.byref(n)) == mbpe.ERR_ARG
    assert n.value == 12 and (out == 77).all() and b"too small" in L.mbpe_last_error()


@pytest.mark.parametrize("K", [0, 1, 2, 5, 9, 17, 40])
@pytest.mark.parametrize("truncation", T.TRUNCATIONS)
def test_plan_equals_the_reference(truncation, K):
    rng = random.Random(K)
    # conversations of 0 .. 7 turns of 0 .. 6 tokens, every flag combination; each (turn_end_id, end_id) setting, heads 0 .. 3
    convs = [[(rng.randrange(7), rng.randrange(4)) for _ in range(rng.randrange(8))] for _ in range(300)]
    docs = [[0] * n for conv in convs for n, _ in conv]
    flags = [f for conv in convs for _, f in conv]
    turn_off = np.concatenate([[0], np.cumsum([len(c) for c in convs])]).astype(np.uint64)
    off = np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.uint64)
    for turn_end_id, end_id in ((None, None), (1, None), (None, 2), (1, 2)):
        for head in range(4):
            kw = dict(max_tokens=K, truncation=truncation, head_turns=head, turn_end_id=turn_end_id, end_id=end_id)
            _, _, want_off, want_info = T.join_all(docs, turn_off, flags, **kw)
            new_off, info = mbpe.turns_plan(off, turn_off, flags, mbpe.turns_spec(**kw))
            assert new_off.tolist() == want_off and info.tolist() == want_info, kw
