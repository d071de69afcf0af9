"""CPU tests of the device planner's entry points (mbpe_pack_fit_plan_device, mbpe_encoder_fit_stats,
mbpe_tok_set_encode_fit_planner): declared, listed and typed; every argument error of mbpe_pack_fit_plan_device has the
code mbpe_pack_fit_plan gives and writes nothing; without a device the call is MBPE_ERR_NO_DEVICE."""
import ctypes
import os
import re

import numpy as np
import pytest

import mbpe
from conftest import ROOT

OFF = [0, 3, 3, 10]


def _spec(seq_len, **kw):
    return mbpe.pack_spec(seq_len, "packed", **kw)


def test_the_new_symbols_are_declared_listed_and_typed():
    L = mbpe.lib()
    header = open(os.path.join(ROOT, "include", "mbpe.h")).read()
    tok_header = open(os.path.join(ROOT, "include", "mbpe_tokenizer.h")).read()
    for s in ("mbpe_pack_fit_plan_device", "mbpe_encoder_fit_stats"):
        assert re.search(r"MBPE_API[^;]*?\b%s\s*\(" % s, header) and s in mbpe.EXPORTS and getattr(L, s).argtypes, s
    s = "mbpe_tok_set_encode_fit_planner"
    assert re.search(r"MBPE_API[^;]*?\b%s\s*\(" % s, tok_header) and s in mbpe.TOK_EXPORTS and getattr(L, s).argtypes
    assert L.mbpe_pack_fit_plan_device.argtypes[1:] == L.mbpe_pack_fit_plan.argtypes
    assert int(re.search(r"#define MBPE_FIT_DEVICE_MAX_SEQ (\d+)u", header).group(1)) == mbpe.FIT_DEVICE_MAX_SEQ >= 8192
    assert hasattr(mbpe.Encoder, "fit_stats") and hasattr(mbpe.Tokenizer, "set_fit_planner")
    with pytest.raises(ValueError):
        mbpe.Tokenizer().set_fit_planner("gpu")
    assert L.mbpe_tok_set_encode_fit_planner(None, 1) == mbpe.ERR_ARG


def test_argument_errors_have_the_host_planners_codes_and_write_nothing():
    L = mbpe.lib()
    o = np.array(OFF, dtype=np.uint64)
    bad = np.array([0, 5, 3, 10], dtype=np.uint64)
    spec = _spec(4)
    ln = np.full(8, 0xABABABAB, dtype=np.uint32)
    drow, dcol = np.full(3, 0xAB, dtype=np.uint64), np.full(3, 0xAB, dtype=np.uint32)
    n = ctypes.c_uint64()
    for off_p, sp, n_out in ((None, spec, n), (o.ctypes.data, None, n), (o.ctypes.data, spec, None),
                             (o.ctypes.data, mbpe.pack_spec(4), n), (bad.ctypes.data, spec, n),
                             (o.ctypes.data, _spec(0), n), (o.ctypes.data, _spec(4, out_bits=8), n)):
        args = (off_p, 3, ctypes.byref(sp) if sp else None, ln.ctypes.data, 8, ctypes.byref(n_out) if n_out is not None else None,
                drow.ctypes.data, dcol.ctypes.data)
        n.value = 77
        want = L.mbpe_pack_fit_plan(*args)
        n.value = 77
        assert L.mbpe_pack_fit_plan_device(0, *args) == want == mbpe.ERR_ARG and (n_out is None or n.value == 0)
    assert (ln == 0xABABABAB).all() and (drow == 0xAB).all() and (dcol == 0xAB).all()


def test_no_device_no_plan():
    import torch
    for device in [1 << 20] + ([] if torch.cuda.is_available() else [0]):
        with pytest.raises(mbpe.MbpeError) as e:
            mbpe.pack_fit_plan(OFF, 4, device=device)
        assert e.value.code == mbpe.ERR_NO_DEVICE
