"""The split rule on code points (csrc/split_rule.h, the device split's option "unicode") against PCRE2, on the CPU:
tests/split_unicode_check.cpp walks texts as the device threads do (same vector, same block) with the class table the
library asked of PCRE2, written to a file here.  The truth is mbpe_presplit on the same bytes.  Required of every
well-formed text, for both patterns:
  - outside the host spans the program's chunk ends are exactly the true ones,
  - every host span starts and ends on a true chunk boundary,
  - no read or write out of bounds: the program runs once plain and once under ASan + UBSan (stand-alone: nothing is
    loaded into Python under a sanitizer),
and where a test says so there is no host span at all.  Of ill-formed text: every ill-formed sequence lies inside a
host span, and the program ends normally.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import mbpe
import split_cases as S
import split_unicode_cases as U
from conftest import read_data

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "minbpe-cc_amd", "csrc")
BLOCK = 64                   # MBPE_SPLIT_BLOCK
DEFAULT_MAX_SPAN = 4096      # MBPE_SPLIT_MAX_SPAN
ENCODERS = ["gpt2", "gpt4"]

FLAGS = {
    "plain": ["-O2"],
    "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
}


@pytest.fixture(scope="module", params=sorted(FLAGS))
def exe(request, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("split_unicode_check_" + request.param) / "split_unicode_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Wextra", "-Werror"] +
                          FLAGS[request.param] + ["-I" + CSRC, os.path.join(HERE, "split_unicode_check.cpp"), "-o", path])
    return path


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    """The library's table as the file the program reads."""
    cls, fold, _ = mbpe.split_unicode_table()
    path = str(tmp_path_factory.mktemp("split_unicode_table") / "table.bin")
    cp = np.zeros(8, dtype=np.uint32)
    to = np.zeros(8, dtype=np.uint8)
    for k, (c, letter) in enumerate(sorted(fold.items())):
        cp[k], to[k] = c, ord(letter)
    with open(path, "wb") as f:
        f.write(cls.tobytes() + np.uint32(len(fold)).tobytes() + cp.tobytes() + to.tobytes())
    return path


def run_check(exe, table, tmp_path, encoder, max_span, blob, off, cuts=()):
    """-> (bool[len(blob)] chunk ends of the walked spans, host spans as an array [n_host, 2])."""
    blob = np.ascontiguousarray(blob, dtype=np.uint8)
    off = np.ascontiguousarray(off, dtype=np.uint64)
    cuts = np.ascontiguousarray(cuts, dtype=np.uint64)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(np.uint64(len(off) - 1).tobytes())
        f.write(off.tobytes())
        f.write(np.uint64(len(cuts)).tobytes())
        f.write(cuts.tobytes())
        f.write(blob.tobytes())
    r = subprocess.run([exe, encoder, str(max_span), table, src, dst], capture_output=True, text=True)
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


def compare(exe, table, tmp_path, encoder, max_span, blob, off, key=None, cuts=()):
    """The three requirements; returns the host spans.  A cut ends one text and begins the next."""
    ends, host = run_check(exe, table, tmp_path, encoder, max_span, blob, off, cuts)
    pieces = np.unique(np.concatenate([np.asarray(off, dtype=np.int64), np.asarray(cuts, dtype=np.int64)]))
    if key is None or (encoder, key) not in _TRUTH:
        truth = S.truth_end_mask(S.PATTERNS[encoder], blob, pieces)
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
    assert len(wrong) == 0, "%s: %d chunk ends differ, first at byte %d: %r" % (
        encoder, len(wrong), wrong[0], bytes(blob[max(0, wrong[0] - 24):wrong[0] + 24]))
    text_start = np.zeros(n + 1, dtype=bool)
    text_start[pieces] = True
    a, b = host[:, 0], host[:, 1]
    assert (text_start[a] | truth[np.maximum(a, 1) - 1]).all(), "a host span starts inside a chunk"
    assert truth[b - 1].all(), "a host span ends inside a chunk"
    return host


def no_host_span(host, blob):
    assert len(host) == 0, "%d host spans, the first: %r" % (len(host), bytes(blob[host[0, 0]:host[0, 1]][:200]))


def join(texts):
    off = np.zeros(len(texts) + 1, dtype=np.uint64)
    np.cumsum([len(t) for t in texts], out=off[1:])
    return np.frombuffer(b"".join(texts), dtype=np.uint8), off


def test_table(table):
    cls, fold, ms = mbpe.split_unicode_table()
    print("table built in %.1f ms, fold set %r" % (ms, fold))
    want = {"L": 0, "N": 1, "S": 2, "O": 3}
    for c in range(128):
        ch = chr(c)
        kind = "L" if ch.isascii() and ch.isalpha() else "N" if ch in "0123456789" else "S" if ch in " \t\n\v\f\r" else "O"
        assert (int(cls[c >> 4]) >> (2 * (c & 15))) & 3 == want[kind], c       # split_class below 0x80
    assert fold.get(0x17F) == "s"
    assert 0x212A not in fold                                                  # the Kelvin sign folds to k
    assert all(c >= 0x80 and letter in "sdmtlver" for c, letter in fold.items())
    for c, kind in ((0xE9, "L"), (0x4E2D, "L"), (0xFF11, "N"), (0xB2, "N"), (0xA0, "S"), (0x2028, "S"), (0x85, "S"),
                    (0x3000, "S"), (0x301, "O"), (0x1F600, "O"), (0x20000, "L")):
        assert (int(cls[c >> 4]) >> (2 * (c & 15))) & 3 == want[kind], hex(c)


@pytest.mark.parametrize("encoder", ENCODERS)
def test_every_scalar_value(exe, table, tmp_path, encoder):
    blob, off = U.every_scalar_value()          # 17 texts, one per plane
    ends, host = run_check(exe, table, tmp_path, encoder, DEFAULT_MAX_SPAN, blob, off)
    if (encoder, "planes") not in _TRUTH:
        _TRUTH[(encoder, "planes")] = S.truth_end_mask(S.PATTERNS[encoder], blob, off)
    truth = _TRUTH[(encoder, "planes")]
    no_host_span(host, blob)
    for plane in range(17):
        a, b = int(off[plane]), int(off[plane + 1])
        wrong = np.flatnonzero(truth[a:b] != ends[a:b])
        assert len(wrong) == 0, "plane %d: %d chunk ends differ, first at byte %d: %r" % (
            plane, len(wrong), wrong[0], bytes(blob[a + max(0, wrong[0] - 24):a + wrong[0] + 24]))


@pytest.mark.parametrize("encoder", ENCODERS)
def test_pseudo_scripts(exe, table, tmp_path, encoder):
    scripts = U.pseudo_scripts()
    blob, off = join([scripts[k] for k in sorted(scripts)] + U.whitespace_ends())
    host = compare(exe, table, tmp_path, encoder, DEFAULT_MAX_SPAN, blob, off, key="scripts")
    no_host_span(host, blob)                    # the text without a space included


@pytest.mark.parametrize("encoder", ENCODERS)
def test_alignment(exe, table, tmp_path, encoder):
    blob, off = join(U.alignment())
    no_host_span(compare(exe, table, tmp_path, encoder, DEFAULT_MAX_SPAN, blob, off, key="alignment"), blob)


@pytest.mark.parametrize("encoder", ENCODERS)
@pytest.mark.parametrize("share", [0.08, 0.6])
def test_random_strings(exe, table, tmp_path, encoder, share):
    for alphabet, seed in ((S.HOSTILE, 21), (S.ASCII, 22)):
        blob, off = S.random_strings(seed, 100000, 40, alphabet, S.NON_ASCII, share)
        host = compare(exe, table, tmp_path, encoder, DEFAULT_MAX_SPAN, blob, off, key="strings %d %g" % (seed, share))
        no_host_span(host, blob)


@pytest.mark.parametrize("encoder", ENCODERS)
@pytest.mark.parametrize("name", ["shakespeare.txt", "taylorswift.txt", "sample.txt"])
def test_fixtures(exe, table, tmp_path, encoder, name):
    data = np.frombuffer(read_data(name), dtype=np.uint8)
    host = compare(exe, table, tmp_path, encoder, DEFAULT_MAX_SPAN, data, [0, len(data)], key=name)
    no_host_span(host, data)                    # taylorswift.txt: (0, 0) for the byte rule's (109, 2142)


@pytest.mark.parametrize("encoder", ENCODERS)
def test_every_prefix_of_three_blocks(exe, table, tmp_path, encoder):
    for seed, share in ((31, 0.08), (32, 0.6)):
        text = S.random_text(seed, 3 * BLOCK + 8, S.HOSTILE, S.NON_ASCII, share)
        assert len(text) > 3 * BLOCK
        lengths = [n for n in range(0, 3 * BLOCK + 1) if (text[n] & 0xC0) != 0x80]
        blob = np.concatenate([text[:n] for n in lengths])
        no_host_span(compare(exe, table, tmp_path, encoder, DEFAULT_MAX_SPAN, blob, np.cumsum([0] + lengths)), blob)


@pytest.mark.parametrize("encoder", ENCODERS)
def test_cuts_next_to_characters(exe, table, tmp_path, encoder):
    # a cut at every character boundary of a text, one at a time: each side is a text of its own
    text = S.random_text(33, 2 * BLOCK + 20, S.HOSTILE, S.NON_ASCII, 0.5)
    bounds = [p for p in range(1, len(text)) if (text[p] & 0xC0) != 0x80]
    blob = np.concatenate([text] * len(bounds))
    off = np.arange(len(bounds) + 1, dtype=np.uint64) * np.uint64(len(text))
    cuts = [k * len(text) + p for k, p in enumerate(bounds)]
    no_host_span(compare(exe, table, tmp_path, encoder, DEFAULT_MAX_SPAN, blob, off, cuts=cuts), blob)


@pytest.mark.parametrize("encoder", ENCODERS)
def test_spans_around_max_span(exe, table, tmp_path, encoder):
    max_span = 256
    for body, n_host in U.max_span_texts(max_span):
        data = np.frombuffer(body, dtype=np.uint8)
        host = compare(exe, table, tmp_path, encoder, max_span, data, [0, len(data)])
        assert len(host) == n_host, body[-8:]
    # the limit counts bytes: 128 two-byte letters are walked, 129 are not
    for n, n_host in ((128, 0), (129, 1)):
        data = np.frombuffer("é".encode() * n, dtype=np.uint8)
        assert len(compare(exe, table, tmp_path, encoder, max_span, data, [0, len(data)])) == n_host


@pytest.mark.parametrize("encoder", ENCODERS)
def test_ill_formed(exe, table, tmp_path, encoder):
    cases = U.ill_formed()
    blob, off = join([c[0] for c in cases])
    _, host = run_check(exe, table, tmp_path, encoder, DEFAULT_MAX_SPAN, blob, off)
    for k, (_, lo, hi) in enumerate(cases):
        a, b = int(off[k]) + lo, int(off[k]) + hi
        inside = ((host[:, 0] <= a) & (host[:, 1] >= b)).any()
        assert inside, "text %d: %r is in no host span" % (k, cases[k][0])
    # a cut inside a sequence: both sides are host spans
    for ch in ("é", "中", "\U0001f600"):
        text = ("ab " + ch + " cd").encode()
        for p in range(4, 3 + len(ch.encode())):
            data = np.frombuffer(text, dtype=np.uint8)
            _, host = run_check(exe, table, tmp_path, encoder, DEFAULT_MAX_SPAN, data, [0, len(data)], cuts=[p])
            assert ((host[:, 0] <= 3) & (host[:, 1] == p)).any() and (host[:, 0] == p).any(), (text, p, host)
