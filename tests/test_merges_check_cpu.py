"""mbpe_merges_check: the "trained table" condition -- both sides of merge k below 256 + k, no pair twice -- on the
host alone.  mbpe_train_begin_from asks it of its prior merges before it touches the device."""
import glob
import os
import re

import numpy as np
import pytest

import mbpe
import oracle as O
from conftest import GOLDEN


def _refused(merges):
    with pytest.raises(mbpe.MbpeError) as e:
        mbpe.merges_check(merges)
    assert e.value.code == mbpe.ERR_ARG
    m = re.search(r"merge (\d+)", str(e.value))
    assert m, str(e.value)
    return int(m.group(1))


def test_declared_and_bound():
    for s in ("mbpe_merges_check", "mbpe_train_begin_from", "mbpe_train_from"):
        assert s in mbpe.EXPORTS and hasattr(mbpe.lib(), s), s
    assert "mbpe_tok_train_continue" in mbpe.TOK_EXPORTS and hasattr(mbpe.lib(), "mbpe_tok_train_continue")


def test_accepts_every_golden_model():
    models = sorted(glob.glob(os.path.join(GOLDEN, "*.model")))
    assert len(models) >= 10
    for path in models:
        with open(path, "rb") as f:
            _, _, merges = O.parse_model(f.read())
        assert len(merges) >= 256, path
        mbpe.merges_check(merges)


def test_accepts_empty_and_chains():
    mbpe.merges_check(np.zeros((0, 2), dtype=np.uint32))
    mbpe.merges_check(None)
    mbpe.merges_check([[97, 97]])
    mbpe.merges_check([[97, 98], [256, 99], [257, 256], [255, 258]])      # every side the newest id that exists


def test_rejects_forward_reference():
    assert _refused([[97, 98], [98, 258]]) == 1                           # 258 does not exist before merge 1
    assert _refused([[97, 98], [300, 98], [1, 2]]) == 1
    assert _refused([[1 << 31, 98]]) == 0
    assert _refused([[97, 0xFFFFFFFF]]) == 0


def test_rejects_self_reference():
    assert _refused([[256, 97]]) == 0
    assert _refused([[97, 98], [99, 100], [258, 258]]) == 2


def test_rejects_repeated_pair():
    assert _refused([[97, 98], [98, 97], [97, 98]]) == 2
    assert _refused([[97, 98], [256, 99], [256, 99], [256, 99]]) == 2     # the first repeat is named


def test_first_offence_wins():
    assert _refused([[97, 98], [97, 98], [999, 1]]) == 1
    assert _refused([[97, 98], [999, 1], [97, 98]]) == 1
