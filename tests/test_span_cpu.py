"""The pure arithmetic of csrc/span.h -- span summaries, the fold of the parity scan, r and the carry -- built by the
host compiler into a stand-alone program (tests/span_check.cpp) and run, once plain and once under ASan + UBSan: the
shifts and clzll calls of that code are where undefined behaviour would hide.  No GPU, nothing is loaded into Python."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "minbpe-cc_amd", "csrc")

FLAGS = {
    "plain": ["-O2"],
    "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
}


@pytest.mark.parametrize("build", sorted(FLAGS))
def test_span_arithmetic(build, tmp_path):
    exe = str(tmp_path / "span_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Wextra", "-Werror"] + FLAGS[build] +
                          ["-I" + CSRC, os.path.join(HERE, "span_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    # 11 lengths x (all ones, zeros, two alternating, 28 random) + one string per zero position (1 + 63 + 9 x 64)
    assert r.stdout.strip().endswith("ok: %d strings, 0 failures" % (11 * 32 + 1 + 63 + 9 * 64))
