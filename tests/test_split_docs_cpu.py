"""The rule of mbpe_splitter_split_docs (csrc/split_rule.h: the walk with cuts, the name finder, the host's plan)
against PCRE2, on the CPU: tests/split_docs_check.cpp runs those functions as the device threads and the host do.  The
truth (split_docs_cases.truth) splits every part of every document on its own with mbpe_presplit; the ranges come from
a Python restatement of Tokenizer::split_on_special.  Required, for both patterns:
  - the ranges are the true ones,
  - outside the host spans the program's chunk ends are exactly the true ones,
  - every host span starts and ends on a true chunk boundary, holds no cut, and says whether it ends at one; matched
    by PCRE2 on the subject the device split hands it, it gives the true ends too,
  - no read or write out of bounds: the program runs once plain and once under ASan + UBSan (stand-alone: nothing is
    loaded into Python under a sanitizer).
No GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import mbpe
import split_cases as S
import split_docs_cases as D

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "minbpe-cc_amd", "csrc")
DEFAULT_MAX_SPAN = 4096      # MBPE_SPLIT_MAX_SPAN

FLAGS = {
    "plain": ["-O2"],
    "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
}


@pytest.fixture(scope="module", params=sorted(FLAGS))
def exe(request, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("split_docs_check_" + request.param) / "split_docs_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Wextra", "-Werror"] +
                          FLAGS[request.param] + ["-I" + CSRC, os.path.join(HERE, "split_docs_check.cpp"), "-o", path])
    return path


def run_check(exe, tmp_path, encoder, max_span, blob, off, names):
    """-> (bool[len(blob)] chunk ends of clean spans and ranges, host spans [n_host, 3], ranges [n_ranges, 3])."""
    blob = np.ascontiguousarray(blob, dtype=np.uint8)
    off = np.ascontiguousarray(off, dtype=np.uint64)
    name_off = np.zeros(len(names) + 1, dtype=np.uint64)
    np.cumsum([len(x) for x in names], out=name_off[1:])
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(np.uint64(len(off) - 1).tobytes())
        f.write(off.tobytes())
        f.write(np.uint64(len(names)).tobytes())
        f.write(name_off.tobytes())
        f.write(b"".join(names))
        f.write(blob.tobytes())
    r = subprocess.run([exe, encoder, str(max_span), src, dst], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = np.fromfile(dst, dtype=np.uint64)
    n_ends, n_host, n_ranges = int(out[0]), int(out[1]), int(out[2])
    ends = np.zeros(len(blob), dtype=bool)
    pos = out[3:3 + n_ends].astype(np.int64)
    assert len(np.unique(pos)) == n_ends, "a chunk end was reported twice"
    ends[pos] = True
    at = 3 + n_ends
    host = out[at:at + 3 * n_host].astype(np.int64).reshape(n_host, 3)
    ranges = out[at + 3 * n_host:].astype(np.int64).reshape(n_ranges, 3)
    return ends, host, ranges


_TRUTH = {}     # the truth of the large inputs, computed once for the two builds of the program


def compare(exe, tmp_path, encoder, max_span, blob, off, names, key=None):
    ends, host, ranges = run_check(exe, tmp_path, encoder, max_span, blob, off, names)
    if key is None or (encoder, key) not in _TRUTH:
        t = D.truth(S.PATTERNS[encoder], blob, off, names)
        if key is not None:
            _TRUTH[(encoder, key)] = t
    else:
        t = _TRUTH[(encoder, key)]
    truth, want_ranges, bounds = t
    assert ranges.tolist() == want_ranges.tolist()
    n = len(blob)
    assert (host[:, 0] < host[:, 1]).all() and (host[:, 1] <= n).all()
    cover = np.zeros(n + 1, dtype=np.int64)
    np.add.at(cover, host[:, 0], 1)
    np.add.at(cover, host[:, 1], -1)
    in_host = np.cumsum(cover)[:n]
    assert in_host.max(initial=0) <= 1, "host spans overlap"
    in_host = in_host > 0
    wrong = np.flatnonzero((truth & ~in_host) != ends)
    assert len(wrong) == 0, "%s: %d chunk ends differ, first at byte %d" % (encoder, len(wrong), wrong[0])
    is_bound = np.zeros(n + 1, dtype=bool)
    is_bound[bounds] = True
    a, b = host[:, 0], host[:, 1]
    assert (is_bound[a] | truth[np.maximum(a, 1) - 1]).all(), "a host span starts inside a chunk"
    assert truth[b - 1].all(), "a host span ends inside a chunk"
    inside = np.cumsum(is_bound)
    assert (inside[b - 1] == inside[a]).all(), "a host span holds a cut"
    assert ((b < n) & is_bound[np.minimum(b, n)] == (host[:, 2] != 0)).all(), "wrong 'ends at a cut' flag"
    # the host's part: [a, b) of a span that ends at a cut, else [a, min(b + 1, n)), matched up to b
    if len(host) <= 20000:
        L = mbpe.lib()
        pat = S.PATTERNS[encoder].encode("utf-8")
        arr = np.ascontiguousarray(blob, dtype=np.uint8)
        full = ends.copy()
        for x, y, c in host.tolist():
            stop = y if c else min(y + 1, n)
            h = ctypes.c_void_p()
            assert L.mbpe_presplit(pat, arr.ctypes.data + x, stop - x, ctypes.byref(h)) == 0
            e = np.ctypeslib.as_array(L.mbpe_split_ends(h), shape=(L.mbpe_split_count(h),)).astype(np.int64)
            full[x + e[e <= y - x] - 1] = True
            L.mbpe_split_free(h)
        assert (full == truth).all(), "host spans matched on their subjects differ at %d" % np.flatnonzero(full != truth)[0]
    return host


@pytest.mark.parametrize("encoder", ["gpt2", "gpt4"])
def test_random_strings_as_documents(exe, tmp_path, encoder):
    blob, off = D.string_sets()
    assert len(np.unique(off % 64)) == 64
    host = compare(exe, tmp_path, encoder, DEFAULT_MAX_SPAN, blob, off, [], key="strings")
    assert len(host) > 1000


@pytest.mark.parametrize("encoder", ["gpt2", "gpt4"])
def test_random_strings_with_names(exe, tmp_path, encoder):
    blob, off = D.string_sets(30000)
    names = [b"sd", b" t", b"'", b"\n\n", "é".encode(), b"sdm"]
    compare(exe, tmp_path, encoder, DEFAULT_MAX_SPAN, blob, off, names, key="strings with names")


@pytest.mark.parametrize("encoder", ["gpt2", "gpt4"])
@pytest.mark.parametrize("max_span", [DEFAULT_MAX_SPAN, 1])
@pytest.mark.parametrize("case", D.NAMED, ids=[c[0] for c in D.NAMED])
def test_named_cases(exe, tmp_path, encoder, max_span, case):
    _, docs, names = case
    blob, off = D.join(docs)
    compare(exe, tmp_path, encoder, max_span, blob, off, names)


def test_pair_by_name():
    """"a  " + "b" splits into a, two spaces, b; "a  b" into a, one space, " b" -- the truth itself."""
    for enc in ("gpt2", "gpt4"):
        blob, off = D.join([b"a  ", b"b", b"a  b"])
        mask, _, _ = D.truth(S.PATTERNS[enc], blob, off, [])
        assert np.flatnonzero(mask).tolist() == [0, 2, 3, 4, 5, 7]


def test_ranges_of_the_truth():
    blob, off = D.join([b"x<e>\x0042<e>\x00 7 z", b"ab<", b"e>"])
    _, ranges, _ = D.truth(S.PATTERNS["gpt4"], blob, off, [b"<e>"])
    assert ranges.tolist() == [[1, 3, 0], [4, 3, D.RAW], [7, 3, 0], [10, 5, D.RAW]]
