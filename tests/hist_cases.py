"""The shapes of the token-count tests (csrc/hist.h): lengths around a lane's piece, a span of 1,024 and a workgroup's
tile of 4,096; ids around every power of two from 2^8 to 2^24, which straddles kHistLocalIds whatever power of two it
is; table sizes from 1 to MBPE_MAX_COUNT_IDS; and the reference every test compares with, np.bincount.
tests/hist_check.cpp generates the same shapes for the host restatement."""
import functools

import numpy as np

TILE = 4096                       # positions a workgroup takes at a time (kHistTile): four spans of 1,024
MAX_COUNT_IDS = 1 << 25           # MBPE_MAX_COUNT_IDS

LENGTHS = (0, 1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, (1 << 20) + 3)
EDGE_IDS = tuple(v for k in range(8, 25) for v in ((1 << k) - 1, 1 << k, (1 << k) + 1))
N_IDS = (1, 256, 257, 65536, 65537, 1 << 24, 1 << 25)


def reference(ids, n_ids):
    """-> (counts uint64[n_ids], n_other) of plain ids (bit 31 already cleared)."""
    ids = np.asarray(ids, dtype=np.int64)
    inside = ids[ids < n_ids]
    return np.bincount(inside, minlength=n_ids).astype(np.uint64), int(len(ids) - len(inside))


@functools.lru_cache(maxsize=None)
def edge_tokens(n, seed=0):
    """n ids: the EDGE_IDS in turn between draws below 2^25 + 2 (so some lie beyond every table)."""
    rng = np.random.default_rng(1000 + seed + n)
    t = rng.integers(0, MAX_COUNT_IDS + 2, size=n, dtype=np.int64).astype(np.uint32)
    k = np.arange(0, n, 3)
    t[k] = np.array(EDGE_IDS, dtype=np.uint32)[(k // 3) % len(EDGE_IDS)]
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def zipf_tokens(n, n_ids, seed=0):
    """n ids with a Zipf-like law over n_ids ids: rank r about 1 / r, the low ids dominate as on text."""
    rng = np.random.default_rng(2000 + seed)
    t = np.minimum(np.exp(rng.random(n) * np.log(n_ids)).astype(np.int64) - 1, n_ids - 1).astype(np.uint32)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def uniform_tokens(n, n_ids, seed=0):
    t = np.random.default_rng(3000 + seed).integers(0, n_ids, size=n, dtype=np.int64).astype(np.uint32)
    t.setflags(write=False)
    return t


def flagged(tokens, every=3):
    """The same ids with bit 31 set on every `every`-th token, as a device stream flags chunk ends."""
    t = np.array(tokens, dtype=np.uint32)
    t[::every] |= np.uint32(0x80000000)
    return t
