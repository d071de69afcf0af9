"""CPU tests of the persistent device encoder (mbpe_encoder_* / mbpe_tok_encode_batch_device): the symbols exist,
arguments are checked before any device call, there is no CPU fallback, and the host encode is what it was."""
import ctypes
import hashlib

import numpy as np
import pytest

import mbpe
import oracle as O
from test_tokenizer_cpu import SPECIAL_SAMPLE_TOKENS, _golden_merges
from conftest import read_data

NEW = ("mbpe_encoder_create", "mbpe_encoder_destroy", "mbpe_encoder_encode", "mbpe_encoder_set_option",
       "mbpe_encoder_kernel_ms", "mbpe_encoder_alloc_count", "mbpe_encoder_pass_tokens")
NEW_TOK = ("mbpe_tok_encode_batch_device",)


def _has_gpu():
    import torch
    return torch.cuda.is_available()


def _create(merges, n_merges, out=True, device=0):
    h = ctypes.c_void_p()
    m = None if merges is None else np.ascontiguousarray(merges, dtype=np.uint32)
    rc = mbpe.lib().mbpe_encoder_create(device, None if m is None else m.ctypes.data, n_merges,
                                        ctypes.byref(h) if out else None)
    return rc, h


def test_encoder_entry_points_are_exported():
    L = mbpe.lib()
    for s in NEW + NEW_TOK:
        assert hasattr(L, s), s


def test_encoder_entry_points_are_listed():
    for s in NEW:
        assert s in mbpe.EXPORTS, s
    for s in NEW_TOK:
        assert s in mbpe.TOK_EXPORTS, s


def test_arguments_are_checked_before_the_device():
    L = mbpe.lib()
    m = np.array([[97, 98]], dtype=np.uint32)
    # these hold with and without a GPU: none of them reaches a device call
    assert _create(m, 1, out=False)[0] == mbpe.ERR_ARG                       # no place for the handle
    assert _create(None, 1)[0] == mbpe.ERR_ARG                               # merges NULL with a count
    n, passes, ms = ctypes.c_uint64(77), ctypes.c_uint32(77), ctypes.c_float()
    text = np.frombuffer(b"abab", dtype=np.uint8)
    out = np.zeros(4, dtype=np.uint32)
    assert L.mbpe_encoder_encode(None, text.ctypes.data, 4, 0, None, 0, out.ctypes.data, 4, 32, 0, None,
                                 ctypes.byref(n), ctypes.byref(passes)) == mbpe.ERR_ARG
    assert (n.value, passes.value) == (0, 0) and not out.any()
    assert L.mbpe_encoder_set_option(None, b"piece_bytes", 65536) == mbpe.ERR_ARG
    assert L.mbpe_encoder_kernel_ms(None, ctypes.byref(ms)) == mbpe.ERR_ARG
    assert L.mbpe_encoder_alloc_count(None, ctypes.byref(n)) == mbpe.ERR_ARG
    assert L.mbpe_encoder_pass_tokens(None, None, 0, ctypes.byref(passes)) == mbpe.ERR_ARG
    tok = mbpe.Tokenizer("")
    tok.set_merges(m)
    doc_off = np.array([0, 2, 4], dtype=np.uint64)
    tok_off = np.zeros(3, dtype=np.uint64)
    args = (tok._h, text.ctypes.data, doc_off.ctypes.data, 2, 0)
    assert L.mbpe_tok_encode_batch_device(*args, 0, out.ctypes.data, 4, tok_off.ctypes.data, None) == mbpe.ERR_ARG
    assert L.mbpe_tok_encode_batch_device(*args, -1, out.ctypes.data, 4, tok_off.ctypes.data,
                                          ctypes.byref(n)) == mbpe.ERR_ARG
    assert not out.any() and not tok_off.any()


@pytest.mark.skipif(_has_gpu(), reason="checks the no-device failure path")
def test_no_cpu_fallback():
    m = np.array([[97, 98]], dtype=np.uint32)
    assert _create(m, 1)[0] == mbpe.ERR_NO_DEVICE
    assert _create(None, 0)[0] == mbpe.ERR_NO_DEVICE                         # no merges at all is a valid table
    with pytest.raises(mbpe.MbpeError) as e:
        mbpe.Encoder(m)
    assert e.value.code == mbpe.ERR_NO_DEVICE
    tok = mbpe.Tokenizer("")
    tok.set_merges(m)
    with pytest.raises(mbpe.MbpeError) as e:
        tok.encode_batch([b"abab", b"", b"ab"], device=0)
    assert e.value.code == mbpe.ERR_NO_DEVICE
    with pytest.raises(mbpe.MbpeError) as e:
        tok.encode(b"abab", device=0)
    assert e.value.code == mbpe.ERR_NO_DEVICE
    # the one-shot calls are built on the encoder and keep their code
    with pytest.raises(mbpe.MbpeError) as e:
        mbpe.encode_chunks(b"abab", None, m)
    assert e.value.code == mbpe.ERR_NO_DEVICE


def test_host_encode_is_unchanged():
    # SURVEY 8c digests, as tests/test_tokenizer_cpu.py has them
    tok = mbpe.Tokenizer("")
    tok.set_merges(_golden_merges("shakespeare_basic_lexical_512"))
    enc = tok.encode(read_data("sample.txt"))
    assert len(enc) == 15677
    assert hashlib.sha256(enc.astype("<u4").tobytes()).hexdigest() == \
        "624874b4a8bce9405f0a89ecb7b3e7eeaa94b2a3235e88c05acd6426c05cb409"
    tok = mbpe.Tokenizer(O.GPT4_SPLIT_PATTERN)
    tok.set_merges(_golden_merges("taylorswift_gpt4_lexical_512"))
    enc = tok.encode(read_data("taylorswift.txt"))
    assert len(enc) == 94201
    assert hashlib.sha256(enc.astype("<u4").tobytes()).hexdigest() == \
        "1b82232e30d1972b1b9f8b54080fc8757bcce310b6b8f9de4d63fdd18f034d0d"
    tok = mbpe.Tokenizer(O.GPT4_SPLIT_PATTERN)
    tok.set_special_tokens_from_file(read_data("special1.txt"))
    tok.set_merges(_golden_merges("taylorswift_gpt4_first_512"))
    assert tok.encode(read_data("specialtokensample.txt")).tolist() == SPECIAL_SAMPLE_TOKENS
    assert tok.encode(b"").tolist() == []
