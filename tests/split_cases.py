"""Texts for the split tests (test_split_cpu.py, test_gpu_split.py): seeded, valid UTF-8 throughout -- PCRE2 with
NO_UTF_CHECK is undefined on anything else."""
import ctypes

import numpy as np

import mbpe


class _Patterns(dict):
    """encoder name -> split pattern, asked of the library on first use (it is built after the tests are collected)."""

    def __missing__(self, encoder):
        self[encoder] = mbpe.split_pattern(encoder)
        return self[encoder]


PATTERNS = _Patterns()

# what the two patterns tell apart below 0x80: the contraction letters in both cases, the apostrophe, digits, the six
# whitespace bytes, bytes that look like whitespace and are not (NUL, 0x1C, 0x7F), punctuation, a few other letters
HOSTILE = [bytes([c]) for c in b"sdmtlvreSDMTLVRExyQ''''0189 \t\n\v\f\r  \n\r\x00\x1c\x7f.,!-"]
ASCII = [bytes([c]) for c in range(128)]
# characters that are letters, digits, whitespace or none of them only by their Unicode properties
NON_ASCII = [s.encode("utf-8") for s in ("\u00e9", "\u00a0", "\u2028", "\u0085", "\uff11", "\u017f", "\u212a", "\u0301",
                                           "\u4e2d", "\U0001f600", "\u00b2", "\u3000")]


def random_chars(seed, n_chars, alphabet, extra=(), extra_share=0.0):
    """n_chars characters drawn from alphabet (a share of them from extra) -> (uint8 bytes, offset of every character,
    n_chars + 1 entries)."""
    rng = np.random.default_rng(seed)
    chars = list(alphabet) + list(extra)
    table = np.zeros((len(chars), 4), dtype=np.uint8)
    width = np.zeros(len(chars), dtype=np.int64)
    for k, c in enumerate(chars):
        table[k, :len(c)] = np.frombuffer(c, dtype=np.uint8)
        width[k] = len(c)
    idx = rng.integers(0, len(alphabet), n_chars)
    if extra:
        other = rng.random(n_chars) < extra_share
        idx[other] = len(alphabet) + rng.integers(0, len(extra), int(other.sum()))
    keep = np.arange(4)[None, :] < width[idx][:, None]
    off = np.zeros(n_chars + 1, dtype=np.int64)
    np.cumsum(width[idx], out=off[1:])
    return table[idx][keep], off


def random_strings(seed, n_strings, max_chars, alphabet, extra=(), extra_share=0.0):
    """n_strings strings of 0 .. max_chars characters -> (uint8 blob, n_strings + 1 byte offsets)."""
    rng = np.random.default_rng(seed + 1000003)
    n_of = rng.integers(0, max_chars + 1, n_strings)
    first = np.zeros(n_strings + 1, dtype=np.int64)
    np.cumsum(n_of, out=first[1:])
    blob, char_off = random_chars(seed, int(first[-1]), alphabet, extra, extra_share)
    return blob, char_off[first].astype(np.uint64)


def random_text(seed, n_bytes, alphabet, extra=(), extra_share=0.0):
    """About n_bytes bytes of such characters as one text, cut at a character boundary."""
    blob, off = random_chars(seed, n_bytes, alphabet, extra, extra_share)
    return blob[:off[np.searchsorted(off, n_bytes, side="right") - 1]].copy()


def truth_end_mask(pattern, blob, off):
    """mbpe_presplit of every text blob[off[k]:off[k + 1]] on its own -> bool array over the blob, True where a byte
    is the last of its chunk.  (The C entry points directly: one call per text, hundreds of thousands of texts.)"""
    L = mbpe.lib()
    pat = pattern.encode("utf-8")
    blob = np.ascontiguousarray(blob, dtype=np.uint8)
    out = np.zeros(len(blob), dtype=bool)
    h = ctypes.c_void_p()
    base = blob.ctypes.data
    for k in range(len(off) - 1):
        a, n = int(off[k]), int(off[k + 1]) - int(off[k])
        if n == 0:
            continue
        rc = L.mbpe_presplit(pat, base + a, n, ctypes.byref(h))
        assert rc == 0, L.mbpe_last_error()
        p = L.mbpe_split_offsets(h)
        assert p, "the split left bytes unmatched"
        o = np.ctypeslib.as_array(p, shape=(L.mbpe_split_count(h) + 1,))
        out[a + o[1:].astype(np.int64) - 1] = True
        L.mbpe_split_free(h)
    return out


def end_mask_of(offsets, n):
    """The trainer's end mask (bit i of byte i >> 3: byte i ends a chunk) from n_chunks + 1 offsets, as bool[n]."""
    out = np.zeros(n, dtype=bool)
    o = np.asarray(offsets, dtype=np.int64)
    out[o[1:][o[1:] > o[:-1]] - 1] = True
    return out
