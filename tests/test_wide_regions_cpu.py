"""The regions of the training option "regions": the general cutter of csrc/wide_regions.h passes its stand-alone check
(tests/wide_regions_check.cpp: the whole stream, ascending, chunk ends only, the capacity, and resident_boundary's cut
with 16 regions), plain and under ASan + UBSan."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

HERE = os.path.dirname(os.path.abspath(__file__))
SANITIZED = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


@pytest.mark.parametrize("flags", [["-O2"], SANITIZED], ids=["plain", "sanitized"])
def test_general_region_cutter(flags, tmp_path):
    exe = str(tmp_path / "wide_regions_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags +
                          ["-I" + os.path.join(ROOT, "minbpe-cc_amd", "csrc"), os.path.join(HERE, "wide_regions_check.cpp"),
                           "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert re.search(r"ok: \d+ checks, 0 failures\s*$", r.stdout)
