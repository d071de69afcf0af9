"""CPU tests of the device-split encode path: the new symbols exist and are listed, and the argument checks of
mbpe_encoder_encode_endmask / mbpe_encoder_encode_batch_endmask / mbpe_splitter_split_docs that need no device come
before anything else -- they hold with and without a GPU, even without an encoder (which no machine without a device
can create: the message tells which check refused the call)."""
import ctypes

import numpy as np
import pytest

import mbpe

NEW = ("mbpe_splitter_split_docs", "mbpe_splitter_ranges", "mbpe_splitter_find_ms", "mbpe_encoder_encode_endmask",
       "mbpe_encoder_encode_batch_endmask")


def _has_gpu():
    import torch
    return torch.cuda.is_available()


def test_entry_points_are_exported_and_listed():
    L = mbpe.lib()
    for s in NEW:
        assert hasattr(L, s) and s in mbpe.EXPORTS, s
    assert hasattr(L, "mbpe_tok_set_encode_split") and "mbpe_tok_set_encode_split" in mbpe.TOK_EXPORTS


def _endmask(singles=None, doc_off=None, token_bits=32, n_bytes=16):
    L = mbpe.lib()
    sg = mbpe._singles(singles)
    docs = None if doc_off is None else np.ascontiguousarray(doc_off, dtype=np.uint64)
    n, passes = ctypes.c_uint64(77), ctypes.c_uint32(77)
    out = np.zeros(n_bytes, dtype=np.uint32)
    rc = L.mbpe_encoder_encode_endmask(None, None, n_bytes, None, sg.ctypes.data if len(sg) else None, len(sg),
                                       None if docs is None else docs.ctypes.data, 0 if docs is None else len(docs) - 1,
                                       out.ctypes.data, n_bytes, token_bits, 0, None, ctypes.byref(n),
                                       ctypes.byref(passes))
    assert (n.value, passes.value) == (0, 0) and not out.any()
    return rc, L.mbpe_last_error().decode()


def test_encode_endmask_checks_its_arguments_before_the_device():
    assert _endmask(singles=[(4, 2, 7), (0, 2, 7)]) == (mbpe.ERR_ARG, "mbpe_encoder_encode_endmask: singles must be "
                                                                      "ascending and disjoint")
    rc, msg = _endmask(singles=[(0, 4, 7), (3, 2, 7)])            # overlapping
    assert rc == mbpe.ERR_ARG and "disjoint" in msg
    rc, msg = _endmask(singles=[(15, 2, 7)])                      # out of range
    assert rc == mbpe.ERR_ARG and "out of range" in msg
    rc, msg = _endmask(singles=[(17, 1, 7)])
    assert rc == mbpe.ERR_ARG and "out of range" in msg
    rc, msg = _endmask(singles=[(3, 0, 7)])                       # empty
    assert rc == mbpe.ERR_ARG and "empty" in msg
    rc, msg = _endmask(singles=[(3, 1, 0x7FFFFFFE)])
    assert rc == mbpe.ERR_ARG and "31 bits" in msg
    rc, msg = _endmask(singles=[(3, 1, 65536)], token_bits=16)
    assert rc == mbpe.ERR_VOCAB and "16 bits" in msg
    rc, msg = _endmask(doc_off=[0, 9, 5, 16])
    assert rc == mbpe.ERR_ARG and "doc_off must be ascending" in msg
    rc, msg = _endmask(doc_off=[0, 9, 17])
    assert rc == mbpe.ERR_ARG and "n_bytes" in msg
    rc, msg = _endmask(token_bits=8)
    assert rc == mbpe.ERR_ARG and "token_bits" in msg
    rc, msg = _endmask(singles=[(0, 2, 7), (2, 2, 8)], doc_off=[0, 2, 16])      # valid, but no encoder
    assert rc == mbpe.ERR_ARG and "NULL" in msg


def test_batch_endmask_checks_its_arguments_before_the_device():
    L = mbpe.lib()
    spec = mbpe.pack_spec(8, "padded", 32, 0, None, None, False, False)
    n_rows = ctypes.c_uint64(77)
    docs = np.array([0, 4, 15], dtype=np.uint64)                  # does not end at n_bytes
    rc = L.mbpe_encoder_encode_batch_endmask(None, None, 16, None, None, 0, docs.ctypes.data, 2, ctypes.byref(spec), None, 0,
                                             0, None, ctypes.byref(n_rows), None, None, None)
    assert rc == mbpe.ERR_ARG and "end at n_bytes" in L.mbpe_last_error().decode() and n_rows.value == 0
    rc = L.mbpe_encoder_encode_batch_endmask(None, None, 16, None, None, 0, None, 2, ctypes.byref(spec), None, 0, 0, None,
                                             ctypes.byref(n_rows), None, None, None)
    assert rc == mbpe.ERR_ARG


def test_split_docs_and_the_switch_check_null():
    L = mbpe.lib()
    n = ctypes.c_uint64(77)
    docs = np.array([0, 4], dtype=np.uint64)
    text = np.frombuffer(b"abcd", dtype=np.uint8)
    assert L.mbpe_splitter_split_docs(None, text.ctypes.data, 4, 0, docs.ctypes.data, 1, None, None, 0, None, None, 0, None,
                                      ctypes.byref(n)) == mbpe.ERR_ARG
    assert n.value == 0
    assert L.mbpe_tok_set_encode_split(None, 1) == mbpe.ERR_ARG
    tok = mbpe.Tokenizer("")
    assert L.mbpe_tok_set_encode_split(tok._h, 1) == mbpe.OK
    assert tok.encode(b"abab").tolist() == [97, 98, 97, 98]       # the host encode is not affected


@pytest.mark.skipif(_has_gpu(), reason="checks the no-device failure path")
def test_no_cpu_fallback():
    tok = mbpe.Tokenizer(mbpe.split_pattern("gpt4"))
    with pytest.raises(mbpe.MbpeError) as e:
        tok.encode(b"some text", device=0, device_split=True)
    assert e.value.code == mbpe.ERR_NO_DEVICE
    with pytest.raises(mbpe.MbpeError) as e:                      # a custom pattern: refused before the device is looked for
        mbpe.Tokenizer("").encode(b"some text", device=0, device_split=True)
    assert e.value.code == mbpe.ERR_ARG
