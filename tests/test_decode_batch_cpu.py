"""CPU tests of batch decode on the device (mbpe_decode_batch / mbpe_tok_decode_batch_device): the symbols exist,
arguments and document offsets are checked before any device call, there is no CPU fallback, and the host decode is
what it was."""
import ctypes

import numpy as np
import pytest

import mbpe
from test_tokenizer_cpu import _golden_merges
from conftest import read_data


def _has_gpu():
    import torch
    return torch.cuda.is_available()


def _tok_batch(tok, tokens, off, device=0, n_out=True, byte_off=True):
    t = np.ascontiguousarray(tokens, dtype=np.uint32)
    o = np.ascontiguousarray(off, dtype=np.uint64)
    b = np.zeros(len(o), dtype=np.uint64)
    n = ctypes.c_uint64()
    return mbpe.lib().mbpe_tok_decode_batch_device(tok._h, t.ctypes.data if len(t) else None, o.ctypes.data, len(o) - 1,
                                                   0, device, None, 0, b.ctypes.data if byte_off else None,
                                                   ctypes.byref(n) if n_out else None)


def test_batch_entry_points_are_exported():
    L = mbpe.lib()
    for s in ("mbpe_decode_batch", "mbpe_tok_decode_batch_device", "mbpe_decoder_alloc_count"):
        assert hasattr(L, s), s
    assert "mbpe_decode_batch" in mbpe.EXPORTS and "mbpe_tok_decode_batch_device" in mbpe.TOK_EXPORTS
    for name in ("decode_batch", "decode_batch_device"):
        assert hasattr(mbpe.Decoder, name), name
    assert hasattr(mbpe.Tokenizer, "decode_batch")


def test_decode_batch_null_arguments():
    L = mbpe.lib()
    t = np.array([1, 2], dtype=np.uint32)
    off = np.array([0, 2], dtype=np.uint64)
    b = np.zeros(2, dtype=np.uint64)
    n = ctypes.c_uint64()
    # without a decoder nothing else can be reached on a machine without a GPU; the other NULLs are refused with it too
    assert L.mbpe_decode_batch(None, t.ctypes.data, 2, 32, 0, off.ctypes.data, 1, None, 0, 0, b.ctypes.data,
                               ctypes.byref(n), None) == mbpe.ERR_ARG
    assert L.mbpe_decode_batch(None, t.ctypes.data, 2, 32, 0, off.ctypes.data, 1, None, 0, 0, b.ctypes.data,
                               None, None) == mbpe.ERR_ARG
    assert L.mbpe_decode_batch(None, t.ctypes.data, 2, 32, 0, off.ctypes.data, 1, None, 0, 0, None,
                               ctypes.byref(n), None) == mbpe.ERR_ARG
    assert L.mbpe_decoder_alloc_count(None, ctypes.byref(n)) == mbpe.ERR_ARG


def test_tokenizer_batch_checks_offsets_and_device_before_the_device():
    tok = mbpe.Tokenizer("")
    tok.set_merges(np.array([[97, 98]], dtype=np.uint32))
    t = [97, 256, 98]
    assert _tok_batch(tok, t, [0, 2, 1, 3]) == mbpe.ERR_ARG                  # not ascending
    assert b"ascending" in mbpe.lib().mbpe_last_error()
    assert _tok_batch(tok, t, [1, 2, 3]) == mbpe.ERR_ARG                     # [0] != 0
    assert b"begin at 0" in mbpe.lib().mbpe_last_error()
    # the token count of this call IS [n_docs]: the one way it can disagree with the tokens is to name some of none
    assert _tok_batch(tok, [], [0, 2, 3]) == mbpe.ERR_ARG
    assert _tok_batch(tok, t, [0, 1, 3], device=-1) == mbpe.ERR_ARG
    assert _tok_batch(tok, t, [0, 1, 3], n_out=False) == mbpe.ERR_ARG
    assert _tok_batch(tok, t, [0, 1, 3], byte_off=False) == mbpe.ERR_ARG


@pytest.mark.skipif(_has_gpu(), reason="checks the no-device failure path")
def test_no_cpu_fallback():
    tok = mbpe.Tokenizer("")
    tok.set_merges(np.array([[97, 98]], dtype=np.uint32))
    assert _tok_batch(tok, [97, 256, 98], [0, 1, 1, 3]) == mbpe.ERR_NO_DEVICE
    assert _tok_batch(tok, [], [0]) == mbpe.ERR_NO_DEVICE
    with pytest.raises(mbpe.MbpeError) as e:
        tok.decode_batch([[97, 256], [], [98]], device=0)
    assert e.value.code == mbpe.ERR_NO_DEVICE


def test_host_decode_is_unchanged(capfd):
    tok = mbpe.Tokenizer("")
    tok.set_merges(_golden_merges("shakespeare_basic_lexical_512"))
    data = read_data("sample.txt")
    assert tok.decode(tok.encode(data)) == data
    tok = mbpe.Tokenizer("")
    tok.set_special_tokens_from_file(b"<|x|> 70000\n<|y|> 98\n")
    tok.set_merges(np.array([[97, 98], [256, 99]], dtype=np.uint32))
    capfd.readouterr()
    assert tok.decode([257, 70000, 98, 300, 256, 0xFFFFFFFF]) == b"abc<|x|><|y|>ab"
    err = capfd.readouterr().err
    # (the binding asks for the length first, so every line appears once per call of the C function)
    assert err.splitlines() == ["Warning: Attempted to decode invalid token ID: 300",
                                "Warning: Attempted to decode invalid token ID: 4294967295"] * 2
