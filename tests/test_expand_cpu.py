"""The expansion of the encoder's "dedup" route, without a GPU: the host restatement of csrc/expand.h against a per-chunk
concatenation and dedup_host's unique_of (csrc/dedup.h) against a std::map, as a stand-alone program (plain and under
ASan + UBSan); and the Python shapes of tests/expand_cases.py against themselves."""
import os
import subprocess

import pytest

import dedup_cases as D
import expand_cases as X

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "minbpe-cc_amd", "csrc")

FLAGS = {
    "plain": ["-O2"],
    "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
}


@pytest.mark.parametrize("build", sorted(FLAGS))
def test_expand_host_restatement(build, tmp_path):
    exe = str(tmp_path / "expand_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Wextra", "-Werror"] + FLAGS[build] +
                          ["-I" + CSRC, os.path.join(HERE, "expand_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.strip().endswith("0 failures")


def test_python_expand():
    out, ends = X.expand([[1, 2], [], [7]], [2, 0, 1, 0])
    assert out == [7, 1, 2, 1, 2] and ends == [1, 3, 3, 5]
    assert X.expand([], []) == ([], [])


def test_shapes_are_what_they_say():
    assert len(set(X.distinct_chunks())) == 600 and len(set(X.equal_chunks())) == 1
    for r in range(8):
        chunks = X.residue_chunks(r)
        assert sum(len(c) for c in chunks[:X.SPAN]) == X.SPAN + r
    u, w, _ = D.dedup(X.long_chunks(), max_chunk_bytes=8192)
    assert len(u) == 3 and sorted(w) == [2, 3, 3]
    u, w, _ = D.dedup(X.long_chunks())
    assert len(u) == 5 and w.count(1) == 3
    text, off = X.with_empty_chunks([b"ab", b"c", b"ab", b"d"])
    assert D.chunks_of(text, off) == [b"ab", b"c", b"ab", b"d"] and len(off) - 1 == 4 + 4
