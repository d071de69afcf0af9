"""Splitter::split_spans (host/presplit.cpp) -- the PCRE2 side of the device split -- as a stand-alone program
(tests/split_spans_check.cpp): matches that leave a gap return MBPE_ERR_SPLIT_GAP and write nothing; stretches matched
on their own subjects give the chunk ends of the whole-text split.  Plain and under ASan + UBSan; no GPU, nothing is
loaded into Python under a sanitizer."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOST = os.path.join(ROOT, "minbpe-cc_amd", "host")

FLAGS = {
    "plain": ["-O2"],
    "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
}


@pytest.mark.parametrize("build", sorted(FLAGS))
def test_split_spans(build, tmp_path):
    exe = str(tmp_path / "split_spans_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Wextra"] + FLAGS[build] +
                          ["-I" + os.path.join(ROOT, "include"), "-I" + HOST, os.path.join(HERE, "split_spans_check.cpp"),
                           os.path.join(HOST, "presplit.cpp"), os.path.join(HOST, "errors.cpp"), "-ldl", "-pthread",
                           "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.strip().endswith("ok: 0 failures")
