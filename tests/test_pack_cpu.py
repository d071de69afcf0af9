"""CPU tests of the id-matrix calls (mbpe_pack_tokens, mbpe_unpack_tokens, mbpe_encoder_encode_batch and the Tokenizer's
two): the symbols exist and are listed, every argument error has its code before any device call, and the row count is
answered without a device."""
import ctypes
import os
import re

import numpy as np
import pytest

import mbpe
from conftest import ROOT

NEW = ("mbpe_pack_tokens", "mbpe_unpack_tokens", "mbpe_pack_kernel_ms", "mbpe_encoder_encode_batch",
       "mbpe_encoder_pack_ms")
NEW_TOK = ("mbpe_tok_encode_batch_packed_device", "mbpe_tok_decode_padded_device")


def _has_gpu():
    import torch
    return torch.cuda.is_available()


def test_exports_match_the_headers():
    L = mbpe.lib()
    header = open(os.path.join(ROOT, "include", "mbpe.h")).read()
    declared = set(re.findall(r"MBPE_API[^;]*?\b(mbpe_\w+)\s*\(", header))
    assert declared == set(mbpe.EXPORTS)
    tok_header = open(os.path.join(ROOT, "include", "mbpe_tokenizer.h")).read()
    tok_declared = set(re.findall(r"MBPE_API[^;]*?\b(mbpe_tok_\w+)\s*\(", tok_header))
    assert tok_declared == set(mbpe.TOK_EXPORTS)
    for s in NEW:
        assert s in declared and hasattr(L, s) and getattr(L, s).argtypes, s
    for s in NEW_TOK:
        assert s in tok_declared and hasattr(L, s) and getattr(L, s).argtypes, s
    for name in ("pack_tokens", "unpack_tokens", "pack_spec", "PackSpec"):
        assert hasattr(mbpe, name), name
    assert hasattr(mbpe.Encoder, "encode_batch")
    assert hasattr(mbpe.Tokenizer, "encode_batch_padded") and hasattr(mbpe.Tokenizer, "decode_padded")


def test_the_spec_struct_is_the_headers():
    header = open(os.path.join(ROOT, "include", "mbpe.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} mbpe_pack_spec;", header).group(1)
    fields = re.findall(r"uint32_t\s+(\w+);", body)
    assert fields == [f for f, _ in mbpe.PackSpec._fields_]
    assert ctypes.sizeof(mbpe.PackSpec) == 4 * len(fields)
    assert (mbpe.PACK_PADDED, mbpe.PACK_PACKED, mbpe.NO_TOKEN) == (0, 1, 0xFFFFFFFF)
    assert re.search(r"#define MBPE_PACK_PADDED 0u", header) and re.search(r"#define MBPE_PACK_PACKED 1u", header)
    assert re.search(r"#define MBPE_NO_TOKEN 0xFFFFFFFFu", header)


def _pack(tokens, off, spec, out=True, cap=None, rows_out=True, tokens_null=False, off_null=False, spec_null=False):
    """mbpe_pack_tokens as it is, host to host -> (code, n_rows, ids buffer, len buffer); the buffers are prefilled."""
    t = np.ascontiguousarray(tokens)
    bits = t.dtype.itemsize * 8
    o = np.ascontiguousarray(off, dtype=np.uint64)
    n_docs = len(o) - 1
    ids = np.full(4096, 0xAB, dtype=np.uint8)
    ln = np.full(64, 0xABABABAB, dtype=np.uint32)
    n_rows = ctypes.c_uint64(77)
    rc = mbpe.lib().mbpe_pack_tokens(
        0, None if tokens_null or not len(t) else t.ctypes.data, len(t), bits, 0, None if off_null else o.ctypes.data,
        n_docs, None if spec_null else ctypes.byref(spec), ids.ctypes.data if out else None, 64 if cap is None else cap,
        0, ln.ctypes.data if out else None, ctypes.byref(n_rows) if rows_out else None)
    return rc, n_rows.value, ids, ln


def _untouched(ids, ln):
    return (ids == 0xAB).all() and (ln == 0xABABABAB).all()


T16 = np.arange(10, dtype=np.uint16)
T32 = np.arange(10, dtype=np.uint32)
OFF = [0, 3, 3, 10]


def test_pack_argument_errors_come_before_the_device():
    ok = mbpe.pack_spec(4)
    cases = [
        # NULL arguments
        (dict(rows_out=False), ok, T32, OFF, mbpe.ERR_ARG),
        (dict(tokens_null=True), ok, T32, OFF, mbpe.ERR_ARG),
        (dict(off_null=True), ok, T32, OFF, mbpe.ERR_ARG),
        (dict(spec_null=True), ok, T32, OFF, mbpe.ERR_ARG),
        # a bad offset array
        ({}, ok, T32, [1, 3, 10], mbpe.ERR_ARG),
        ({}, ok, T32, [0, 5, 3, 10], mbpe.ERR_ARG),
        ({}, ok, T32, [0, 3, 9], mbpe.ERR_ARG),
        ({}, ok, T32, [0, 3, 11], mbpe.ERR_ARG),
        # the spec
        ({}, mbpe.pack_spec(0), T32, OFF, mbpe.ERR_ARG),
        ({}, mbpe.pack_spec(0, "packed"), T32, OFF, mbpe.ERR_ARG),
        ({}, mbpe.pack_spec(1, bos_id=1, eos_id=2), T32, OFF, mbpe.ERR_ARG),
        ({}, mbpe.pack_spec(0, bos_id=1), T32, OFF, mbpe.ERR_ARG),
        ({}, mbpe.pack_spec(4, layout=2), T32, OFF, mbpe.ERR_ARG),
        ({}, mbpe.pack_spec(4, layout=0xFFFFFFFF), T32, OFF, mbpe.ERR_ARG),
        ({}, mbpe.pack_spec(4, out_bits=8), T32, OFF, mbpe.ERR_ARG),
        ({}, mbpe.pack_spec(4, out_bits=0), T32, OFF, mbpe.ERR_ARG),
        ({}, mbpe.pack_spec(4, out_bits=24), T16, OFF, mbpe.ERR_ARG),
        ({}, mbpe.pack_spec(4, out_bits=128), T16, OFF, mbpe.ERR_ARG),
        ({}, mbpe.pack_spec(4, "packed", pad_left=True), T32, OFF, mbpe.ERR_ARG),
        ({}, mbpe.pack_spec(4, "packed", trunc_left=True), T32, OFF, mbpe.ERR_ARG),
        # what does not fit 16 bits
        ({}, mbpe.pack_spec(4, out_bits=16), T32, OFF, mbpe.ERR_VOCAB),
        ({}, mbpe.pack_spec(4, "packed", out_bits=16), T32, OFF, mbpe.ERR_VOCAB),
        ({}, mbpe.pack_spec(4, out_bits=16, pad_id=65536), T16, OFF, mbpe.ERR_VOCAB),
        ({}, mbpe.pack_spec(4, out_bits=16, bos_id=65536), T16, OFF, mbpe.ERR_VOCAB),
        ({}, mbpe.pack_spec(4, out_bits=16, eos_id=1 << 20), T16, OFF, mbpe.ERR_VOCAB),
        ({}, mbpe.pack_spec(4, "packed", out_bits=16, eos_id=65536), T16, OFF, mbpe.ERR_VOCAB),
    ]
    for kw, spec, tokens, off, want in cases:
        rc, n_rows, ids, ln = _pack(tokens, off, spec, **kw)
        assert rc == want, (kw, list(bytes(spec)), off, rc)
        if kw.get("rows_out", True):
            assert n_rows == 0
        assert _untouched(ids, ln)
        assert mbpe.lib().mbpe_last_error()
    # token_bits is neither 16 nor 32
    n_rows = ctypes.c_uint64(77)
    o = np.array(OFF, dtype=np.uint64)
    for bits in (0, 8, 31, 64):
        assert mbpe.lib().mbpe_pack_tokens(0, T32.ctypes.data, 10, bits, 0, o.ctypes.data, 3, ctypes.byref(ok), None, 0, 0,
                                           None, ctypes.byref(n_rows)) == mbpe.ERR_ARG
        assert n_rows.value == 0


def test_the_row_count_needs_no_device():
    for spec, tokens, want in [
        (mbpe.pack_spec(4), T32, 3),
        (mbpe.pack_spec(1, out_bits=64), T16, 3),
        (mbpe.pack_spec(4, "packed"), T32, 3),                       # 10 ids
        (mbpe.pack_spec(5, "packed"), T32, 2),
        (mbpe.pack_spec(5, "packed", bos_id=1), T32, 3),             # 13 ids
        (mbpe.pack_spec(4, "packed", bos_id=1, eos_id=2, out_bits=16), T16, 4),      # 16 ids
        (mbpe.pack_spec(3, "packed", bos_id=1, eos_id=2, out_bits=16), T16, 6),
        (mbpe.pack_spec(1, "packed", bos_id=1, eos_id=2), T32, 16),   # seq_len below nb + ne is fine when PACKED
        (mbpe.pack_spec(2, bos_id=1, eos_id=2), T32, 3),             # and seq_len == nb + ne when PADDED
        (mbpe.pack_spec(4, out_bits=16, pad_id=65535, bos_id=65535, eos_id=65535), T16, 3),
    ]:
        rc, n_rows, ids, ln = _pack(tokens, OFF, spec, out=False)
        assert (rc, n_rows) == (mbpe.OK, want) and _untouched(ids, ln), list(bytes(spec))
        rc, n_rows, ids, ln = _pack(tokens, OFF, spec, cap=want - 1)       # too small: the count, nothing written
        assert (rc, n_rows) == (mbpe.ERR_ARG, want) and _untouched(ids, ln), list(bytes(spec))
        assert b"too small" in mbpe.lib().mbpe_last_error()
    empty = np.zeros(0, dtype=np.uint32)
    for layout in ("padded", "packed"):
        for off, want in (([0], 0), ([0, 0, 0], 2 if layout == "padded" else 0)):
            rc, n_rows, ids, ln = _pack(empty, off, mbpe.pack_spec(4, layout), out=False)
            assert (rc, n_rows) == (mbpe.OK, want)
    # nothing to write is no device call either
    rc, n_rows, ids, ln = _pack(empty, [0], mbpe.pack_spec(4))
    assert (rc, n_rows) == (mbpe.OK, 0) and _untouched(ids, ln)
    ids, lengths = mbpe.pack_tokens(empty, [0], 4, "packed", out_bits=64)
    assert ids.shape == (0, 4) and ids.dtype == np.uint64 and lengths.shape == (0,)


def _unpack(ids, lengths, seq_len, id_bits=32, token_bits=32, out=True, cap=64, n_null=False, ids_null=False,
            len_null=False):
    m = np.ascontiguousarray(ids)
    ln = np.ascontiguousarray(lengths, dtype=np.uint32)
    n_rows = len(ln)
    tok = np.full(64, 0xABABABAB, dtype=np.uint32)
    off = np.full(n_rows + 1, 0x5555555555555555, dtype=np.uint64)
    n = ctypes.c_uint64(77)
    rc = mbpe.lib().mbpe_unpack_tokens(0, None if ids_null else m.ctypes.data, n_rows, seq_len, id_bits, 0,
                                       None if len_null else ln.ctypes.data, tok.ctypes.data if out else None, cap,
                                       token_bits, 0, off.ctypes.data, None if n_null else ctypes.byref(n))
    return rc, n.value, tok, off


def test_unpack_argument_errors_and_query():
    m = np.arange(12, dtype=np.uint32).reshape(3, 4)
    fresh = lambda tok: (tok == 0xABABABAB).all()
    for kw, want in [
        (dict(n_null=True), mbpe.ERR_ARG), (dict(ids_null=True), mbpe.ERR_ARG), (dict(len_null=True), mbpe.ERR_ARG),
        (dict(id_bits=8), mbpe.ERR_ARG), (dict(id_bits=24), mbpe.ERR_ARG), (dict(token_bits=64), mbpe.ERR_ARG),
        (dict(token_bits=8), mbpe.ERR_ARG), (dict(seq_len=0), mbpe.ERR_ARG),
        (dict(token_bits=16), mbpe.ERR_VOCAB), (dict(id_bits=64, token_bits=16), mbpe.ERR_VOCAB),
    ]:
        kw.setdefault("seq_len", 4)
        rc, n, tok, off = _unpack(m, [4, 0, 2], **kw)
        assert rc == want and fresh(tok), kw
        if not kw.get("n_null"):
            assert n == 0
    # a length beyond seq_len is refused, with the row named
    for lengths in ([5, 0, 2], [4, 0, 0xFFFFFFFF]):
        rc, n, tok, off = _unpack(m, lengths, 4)
        assert (rc, n) == (mbpe.ERR_ARG, 0) and fresh(tok)
        assert b"seq_len" in mbpe.lib().mbpe_last_error()
    # the query and the cap rule, without a device
    rc, n, tok, off = _unpack(m, [4, 0, 2], 4, out=False)
    assert (rc, n) == (mbpe.OK, 6) and off.tolist() == [0, 4, 4, 6]
    rc, n, tok, off = _unpack(m, [4, 0, 2], 4, cap=5)
    assert (rc, n) == (mbpe.ERR_ARG, 6) and fresh(tok) and off.tolist() == [0, 4, 4, 6]
    rc, n, tok, off = _unpack(m, [0, 0, 0], 4)
    assert (rc, n) == (mbpe.OK, 0) and fresh(tok) and off.tolist() == [0, 0, 0, 0]
    ms = ctypes.c_float(-1.0)
    assert mbpe.lib().mbpe_pack_kernel_ms(None) == mbpe.ERR_ARG
    assert mbpe.lib().mbpe_pack_kernel_ms(ctypes.byref(ms)) == mbpe.OK and ms.value >= 0.0


def test_encoder_and_tokenizer_entry_points_check_their_arguments():
    L = mbpe.lib()
    spec = mbpe.pack_spec(4)
    text = np.frombuffer(b"abab", dtype=np.uint8)
    docs = np.array([0, 1], dtype=np.uint64)
    ids = np.full(16, 0xABABABAB, dtype=np.uint32)
    ln = np.full(4, 0xABABABAB, dtype=np.uint32)
    n_rows, n_tok, ms = ctypes.c_uint64(77), ctypes.c_uint64(77), ctypes.c_float()
    assert L.mbpe_encoder_encode_batch(None, text.ctypes.data, 4, 0, None, 0, docs.ctypes.data, 1, ctypes.byref(spec),
                                       ids.ctypes.data, 4, 0, ln.ctypes.data, ctypes.byref(n_rows),
                                       ctypes.byref(n_tok)) == mbpe.ERR_ARG
    assert (n_rows.value, n_tok.value) == (0, 0)
    assert L.mbpe_encoder_pack_ms(None, ctypes.byref(ms)) == mbpe.ERR_ARG
    tok = mbpe.Tokenizer("")
    tok.set_merges(np.array([[97, 98]], dtype=np.uint32))
    doc_off = np.array([0, 2, 4], dtype=np.uint64)
    head = (tok._h, text.ctypes.data, doc_off.ctypes.data, 2, 0)
    tail = (ids.ctypes.data, 4, 0, ln.ctypes.data)
    n_rows.value = 77
    assert L.mbpe_tok_encode_batch_packed_device(*head, -1, ctypes.byref(spec), *tail, ctypes.byref(n_rows),
                                                 None) == mbpe.ERR_ARG
    assert n_rows.value == 0
    assert L.mbpe_tok_encode_batch_packed_device(*head, 0, None, *tail, ctypes.byref(n_rows), None) == mbpe.ERR_ARG
    assert L.mbpe_tok_encode_batch_packed_device(*head, 0, ctypes.byref(spec), *tail, None, None) == mbpe.ERR_ARG
    bad = np.array([0, 3, 2], dtype=np.uint64)
    assert L.mbpe_tok_encode_batch_packed_device(tok._h, text.ctypes.data, bad.ctypes.data, 2, 0, 0, ctypes.byref(spec),
                                                 *tail, ctypes.byref(n_rows), None) == mbpe.ERR_ARG
    # a length beyond seq_len is refused where there is no device, too: before a decoder is created
    m = np.arange(8, dtype=np.uint32).reshape(2, 4)
    lengths = np.array([4, 5], dtype=np.uint32)
    byte_off = np.zeros(3, dtype=np.uint64)
    n = ctypes.c_uint64(77)
    assert L.mbpe_tok_decode_padded_device(tok._h, m.ctypes.data, 2, 4, lengths.ctypes.data, 0, 0, None, 0,
                                           byte_off.ctypes.data, ctypes.byref(n)) == mbpe.ERR_ARG
    assert n.value == 0 and b"seq_len" in L.mbpe_last_error()
    assert L.mbpe_tok_decode_padded_device(tok._h, m.ctypes.data, 2, 4, lengths.ctypes.data, 0, -1, None, 0,
                                           byte_off.ctypes.data, ctypes.byref(n)) == mbpe.ERR_ARG
    assert L.mbpe_tok_decode_padded_device(tok._h, m.ctypes.data, 2, 4, lengths.ctypes.data, 0, 0, None, 0, None,
                                           ctypes.byref(n)) == mbpe.ERR_ARG
    assert (ids == 0xABABABAB).all() and (ln == 0xABABABAB).all()
    with pytest.raises(ValueError):
        mbpe.pack_spec(4, layout="ragged")
    tok.close()


@pytest.mark.skipif(_has_gpu(), reason="checks the no-device failure path")
def test_no_cpu_fallback():
    rc, n_rows, ids, ln = _pack(T32, OFF, mbpe.pack_spec(4))
    assert (rc, n_rows) == (mbpe.ERR_NO_DEVICE, 3) and _untouched(ids, ln)
    rc, n, tok, off = _unpack(np.arange(12, dtype=np.uint32).reshape(3, 4), [4, 0, 2], 4)
    assert (rc, n) == (mbpe.ERR_NO_DEVICE, 6) and (tok == 0xABABABAB).all()
    with pytest.raises(mbpe.MbpeError) as e:
        mbpe.pack_tokens(T32, OFF, 4)
    assert e.value.code == mbpe.ERR_NO_DEVICE
    tok = mbpe.Tokenizer("")
    tok.set_merges(np.array([[97, 98]], dtype=np.uint32))
    with pytest.raises(mbpe.MbpeError) as e:
        tok.encode_batch_padded([b"abab", b"", b"ab"], 4)
    assert e.value.code == mbpe.ERR_NO_DEVICE
    with pytest.raises(mbpe.MbpeError) as e:
        tok.decode_padded(np.zeros((2, 4), dtype=np.uint32), [1, 2])
    assert e.value.code == mbpe.ERR_NO_DEVICE
    tok.close()
