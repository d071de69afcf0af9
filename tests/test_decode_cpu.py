"""CPU tests of decode on the device (mbpe_decoder_create / mbpe_decode_tokens / mbpe_decode_stream /
mbpe_tok_decode_device): the symbols exist, arguments are checked before any device call, there is no CPU
fallback, and the host decode is what it was."""
import ctypes

import numpy as np
import pytest

import mbpe
from test_tokenizer_cpu import _golden_merges
from conftest import read_data


def _has_gpu():
    import torch
    return torch.cuda.is_available()


def _create(merges, n_merges, ids=None, blob=None, off=None, n_special=0, out=True):
    h = ctypes.c_void_p()
    keep = [np.ascontiguousarray(a) if a is not None else None for a in (merges, ids, blob, off)]
    ptr = [None if a is None else a.ctypes.data for a in keep]
    rc = mbpe.lib().mbpe_decoder_create(0, ptr[0], n_merges, ptr[1], ptr[2], ptr[3], n_special,
                                        ctypes.byref(h) if out else None)
    return rc, h


def test_decode_entry_points_are_exported():
    L = mbpe.lib()
    for s in ("mbpe_decoder_create", "mbpe_decoder_destroy", "mbpe_decode_tokens", "mbpe_decode_stream",
              "mbpe_decode_slots", "mbpe_encode_chunks_device", "mbpe_tok_decode_device"):
        assert hasattr(L, s), s
    assert "mbpe_decode_tokens" in mbpe.EXPORTS and "mbpe_tok_decode_device" in mbpe.TOK_EXPORTS


def test_arguments_are_checked_before_the_device():
    m = np.array([[97, 98]], dtype=np.uint32)
    # these hold with and without a GPU: none of them reaches a device call
    assert _create(m, 1, out=False)[0] == mbpe.ERR_ARG                       # no place for the handle
    assert _create(None, 1)[0] == mbpe.ERR_ARG                               # merges NULL
    assert _create(m, 1, None, None, None, 1)[0] == mbpe.ERR_ARG             # specials NULL
    ids = np.array([300, 301], dtype=np.uint32)
    blob = np.frombuffer(b"abcdef", dtype=np.uint8)
    assert _create(m, 1, ids, blob, np.array([0, 4, 2], dtype=np.uint64), 2)[0] == mbpe.ERR_ARG   # descending
    assert b"ascending" in mbpe.lib().mbpe_last_error()
    assert _create(m, (1 << 24) - 256 + 1)[0] == mbpe.ERR_ARG                # beyond MBPE_MAX_VOCAB_WIDE - 256
    n = ctypes.c_uint64()
    t = np.array([1, 2], dtype=np.uint32)
    assert mbpe.lib().mbpe_decode_tokens(None, t.ctypes.data, 2, 0, None, 0, 0, ctypes.byref(n), None) == mbpe.ERR_ARG
    assert mbpe.lib().mbpe_decode_stream(None, None, 0, 0, ctypes.byref(n)) == mbpe.ERR_ARG
    assert mbpe.lib().mbpe_decode_slots(None, None, 0, 16, 0, 0xFFFFFFFF, None, 0, 1, ctypes.byref(n), None) == mbpe.ERR_ARG
    tok = mbpe.Tokenizer("")
    assert mbpe.lib().mbpe_tok_decode_device(tok._h, t.ctypes.data, 2, 0, -1, None, 0, ctypes.byref(n)) == mbpe.ERR_ARG
    assert mbpe.lib().mbpe_tok_decode_device(tok._h, t.ctypes.data, 2, 0, 0, None, 0, None) == mbpe.ERR_ARG


def test_vocabulary_beyond_the_caps_is_refused_before_the_device():
    # (97,97), (256,256), ...: entry 256 + k holds 2^(k+1) bytes; 2^22 exceeds MBPE_DECODER_MAX_ENTRY
    m = np.array([[97, 97]] + [[255 + k, 255 + k] for k in range(1, 22)], dtype=np.uint32)
    assert _create(m, len(m))[0] == mbpe.ERR_OOM
    assert b"MBPE_DECODER_MAX_ENTRY" in mbpe.lib().mbpe_last_error()
    # lengths that would wrap 64 bits if they were summed blindly
    m = np.array([[97, 97]] + [[255 + k, 255 + k] for k in range(1, 80)], dtype=np.uint32)
    assert _create(m, len(m))[0] == mbpe.ERR_OOM


@pytest.mark.skipif(_has_gpu(), reason="checks the no-device failure path")
def test_no_cpu_fallback():
    m = np.array([[97, 98]], dtype=np.uint32)
    assert _create(m, 1)[0] == mbpe.ERR_NO_DEVICE
    with pytest.raises(mbpe.MbpeError) as e:
        mbpe.Decoder(m)
    assert e.value.code == mbpe.ERR_NO_DEVICE
    tok = mbpe.Tokenizer("")
    tok.set_merges(m)
    with pytest.raises(mbpe.MbpeError) as e:
        tok.decode([97, 256], device=0)
    assert e.value.code == mbpe.ERR_NO_DEVICE
    with pytest.raises(mbpe.MbpeError) as e:
        mbpe.encode_chunks_device(b"abab", None, m, 0, 0)
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
    assert err.count("Warning: Attempted to decode invalid token ID: 300\n") == 2
    assert err.count("Warning: Attempted to decode invalid token ID: 4294967295\n") == 2
