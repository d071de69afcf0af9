"""The run before a tile without a GPU: run_before_tile of csrc/run_before.h, the host form of the walk that a split pass
uses instead of the run scan, against a restatement of that scan (tests/run_before_check.cpp) over hand-built and random
summary arrays, as a stand-alone program -- plain, and under ASan + UBSan."""
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
def test_run_before_tile_against_the_scan(build, tmp_path):
    exe = str(tmp_path / "run_before_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Wextra", "-Werror"] + FLAGS[build] +
                          ["-I" + CSRC, os.path.join(HERE, "run_before_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.strip().endswith("0 failures")


def test_the_library_is_built_from_the_header():
    """The header is one of the sources whose hash the library carries: a change to it rebuilds the library."""
    import __graft_entry__ as G
    assert any(os.path.basename(p) == "run_before.h" for p in G.LIB_DEPS)
