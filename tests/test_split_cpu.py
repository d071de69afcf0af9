"""The split rule of csrc/split_rule.h against PCRE2, on the CPU: tests/split_check.cpp walks texts as the device
threads do (same vector, same block) and reports the chunk ends of the clean spans and the host spans; the truth is
mbpe_presplit on the same bytes.  Required of every text, for both patterns:
  - outside the host spans the program's chunk ends are exactly the true ones,
  - every host span starts and ends on a true chunk boundary,
  - no read or write out of bounds: the program runs once plain and once under ASan + UBSan (stand-alone: nothing is
    loaded into Python under a sanitizer).
No GPU."""
import os
import subprocess

import numpy as np
import pytest

import split_cases as S
from conftest import read_data

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "minbpe-cc_amd", "csrc")
BLOCK = 64                   # MBPE_SPLIT_BLOCK
DEFAULT_MAX_SPAN = 4096      # MBPE_SPLIT_MAX_SPAN

FLAGS = {
    "plain": ["-O2"],
    "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
}


@pytest.fixture(scope="module", params=sorted(FLAGS))
def exe(request, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("split_check_" + request.param) / "split_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Wextra", "-Werror"] +
                          FLAGS[request.param] + ["-I" + CSRC, os.path.join(HERE, "split_check.cpp"), "-o", path])
    return path


def run_check(exe, tmp_path, encoder, max_span, blob, off):
    """-> (bool[len(blob)] chunk ends of the clean spans, host spans as an array [n_host, 2])."""
    blob = np.ascontiguousarray(blob, dtype=np.uint8)
    off = np.ascontiguousarray(off, dtype=np.uint64)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(np.uint64(len(off) - 1).tobytes())
        f.write(off.tobytes())
        f.write(blob.tobytes())
    r = subprocess.run([exe, encoder, str(max_span), src, dst], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = np.fromfile(dst, dtype=np.uint64)
    n_ends, n_host = int(out[0]), int(out[1])
    ends = np.zeros(len(blob), dtype=bool)
    pos = out[2:2 + n_ends].astype(np.int64)
    assert len(np.unique(pos)) == n_ends, "a chunk end was reported twice"
    ends[pos] = True
    return ends, out[2 + n_ends:].astype(np.int64).reshape(n_host, 2)


_TRUTH = {}     # the truth of the large inputs, computed once for the two builds of the program


def compare(exe, tmp_path, encoder, max_span, blob, off, key=None):
    """The three requirements; returns the host spans."""
    ends, host = run_check(exe, tmp_path, encoder, max_span, blob, off)
    if key is None or (encoder, key) not in _TRUTH:
        truth = S.truth_end_mask(S.PATTERNS[encoder], blob, off)
        if key is not None:
            _TRUTH[(encoder, key)] = truth
    else:
        truth = _TRUTH[(encoder, key)]
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
    # a host span starts at the start of its text or right behind a true chunk end, and ends right behind one
    text_start = np.zeros(n + 1, dtype=bool)
    text_start[np.asarray(off, dtype=np.int64)] = True
    a, b = host[:, 0], host[:, 1]
    assert (text_start[a] | truth[np.maximum(a, 1) - 1]).all(), "a host span starts inside a chunk"
    assert truth[b - 1].all(), "a host span ends inside a chunk"
    return host


@pytest.mark.parametrize("encoder", ["gpt2", "gpt4"])
@pytest.mark.parametrize("alphabet", ["hostile", "ascii"])
def test_random_ascii_strings(exe, tmp_path, encoder, alphabet):
    # 2 x 100,000 strings of up to 40 bytes; pure ASCII, so everything is walked by the rule
    blob, off = S.random_strings(11 if alphabet == "hostile" else 12, 100000, 40,
                                 S.HOSTILE if alphabet == "hostile" else S.ASCII)
    host = compare(exe, tmp_path, encoder, DEFAULT_MAX_SPAN, blob, off, key="ascii strings " + alphabet)
    assert len(host) == 0


@pytest.mark.parametrize("encoder", ["gpt2", "gpt4"])
@pytest.mark.parametrize("alphabet", ["hostile", "ascii"])
def test_random_strings_with_non_ascii(exe, tmp_path, encoder, alphabet):
    blob, off = S.random_strings(21 if alphabet == "hostile" else 22, 100000, 40,
                                 S.HOSTILE if alphabet == "hostile" else S.ASCII, S.NON_ASCII, 0.08)
    host = compare(exe, tmp_path, encoder, DEFAULT_MAX_SPAN, blob, off, key="non-ascii strings " + alphabet)
    assert len(host) > 10000


@pytest.mark.parametrize("encoder", ["gpt2", "gpt4"])
@pytest.mark.parametrize("name,n_host,host_bytes", [("shakespeare.txt", 0, 0), ("taylorswift.txt", 109, 2142),
                                                    ("sample.txt", None, None)])
def test_fixtures(exe, tmp_path, encoder, name, n_host, host_bytes):
    data = np.frombuffer(read_data(name), dtype=np.uint8)
    host = compare(exe, tmp_path, encoder, DEFAULT_MAX_SPAN, data, [0, len(data)])
    if n_host is not None:
        assert len(host) == n_host
        assert int((host[:, 1] - host[:, 0]).sum()) == host_bytes


@pytest.mark.parametrize("encoder", ["gpt2", "gpt4"])
def test_every_prefix_of_three_blocks(exe, tmp_path, encoder):
    for seed, extra in ((31, ()), (32, S.NON_ASCII)):
        text = S.random_text(seed, 3 * BLOCK + 8, S.HOSTILE, extra, 0.08)
        assert len(text) > 3 * BLOCK
        # every prefix of 0 .. 3 blocks that ends on a character boundary
        lengths = [n for n in range(0, 3 * BLOCK + 1) if (text[n] & 0xC0) != 0x80]
        blob = np.concatenate([text[:n] for n in lengths])
        compare(exe, tmp_path, encoder, DEFAULT_MAX_SPAN, blob, np.cumsum([0] + lengths))


@pytest.mark.parametrize("encoder", ["gpt2", "gpt4"])
def test_long_runs_around_max_span(exe, tmp_path, encoder):
    max_span = 256
    texts = []
    for fill in (b"a", b"1", b" "):
        for n in (max_span - 1, max_span, max_span + 1, 3 * max_span + 5):
            texts += [fill * n, b"ab " + fill * n, b"ab " + fill * n + b" cd\n", fill * n + b"\n\nx"]
    off = np.cumsum([0] + [len(t) for t in texts])
    host = compare(exe, tmp_path, encoder, max_span, np.frombuffer(b"".join(texts), dtype=np.uint8), off)
    # a span of exactly max_span bytes is walked, one byte more goes to the host
    for fill in (b"a", b"1"):
        assert len(compare(exe, tmp_path, encoder, max_span, np.frombuffer(fill * max_span, np.uint8), [0, max_span])) == 0
        assert len(compare(exe, tmp_path, encoder, max_span, np.frombuffer(fill * (max_span + 1), np.uint8),
                           [0, max_span + 1])) == 1
    assert len(host) > 0
    # one span of max_span + 2 bytes, the digits not at its start
    text = b"x" + b"1" * (max_span + 1)
    assert compare(exe, tmp_path, encoder, max_span, np.frombuffer(text, np.uint8), [0, len(text)]).tolist() == [[0, len(text)]]
