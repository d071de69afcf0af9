"""The pure arithmetic of csrc/rank.h -- the summaries of the segmented minimum, their fold, the in-group scan steps on
end-flag masks, the carries of the sweeps -- built by the host compiler into a stand-alone program
(tests/rank_check.cpp) and run, once plain and once under ASan + UBSan: the shifts, clzll and ctzll calls of that code
are where undefined behaviour would hide.  No GPU, nothing is loaded into Python."""
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
def test_rank_arithmetic(build, tmp_path):
    exe = str(tmp_path / "rank_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Wextra", "-Werror"] + FLAGS[build] +
                          ["-I" + CSRC, os.path.join(HERE, "rank_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    # 11 lengths x (1 without anything, 3 x 2 with one minimum, 6 regular, 28 random) + two strings per end-flag
    # position: the first group (1 + 63 + 9 x 64 positions) and the last group of the first span (63 + 6 x 64)
    assert r.stdout.strip().endswith("ok: %d strings, 0 failures" % (11 * 41 + 2 * (1 + 63 + 9 * 64) + 2 * (63 + 6 * 64)))
