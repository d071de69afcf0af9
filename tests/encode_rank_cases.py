"""Rank-ordered encode (option "rank_order" of csrc/encode.hip, Tokenizer.encode(order="rank")): a pure-Python
reference and case generators.  No GPU, no product code.

The definition, per chunk, after text_to_vector: of the adjacent pairs that are in merges_lookup (a repeated pair keeps
the last id) take the smallest id m; stop if there is none; replace every occurrence of that pair with m, left to right
and non-overlapping; repeat.  Three restatements:
  rank_loop_chunk   the loop as it is written above, on a Python list (small inputs)
  replay_chunk      merges 0 .. n-1 applied in order: equal to the loop for a well-formed table (both sides of merge k
                    below 256 + k, no pair twice), and the trainer's own segmentation
  rank_loop_text    the loop over all chunks of a text at once, in numpy (the large inputs of the GPU tests); it also
                    counts the passes and the tokens that enter each, which the device reports
The generators lay chunks, minima and runs around the kernels' units: groups of 64 lanes, spans of 1,024 tokens and the
slices of ceil(n_spans / 1,024) spans that a thread of the scans owns (encode_cases.geometry)."""
from collections import namedtuple

import numpy as np

import encode_cases as E
from test_bruteforce_cpu import text_to_vector

NONE = 0xFFFFFFFF

# singles: None, or rows (start, len, id) -- byte ranges that are one token each (mbpe_encoder_encode_endmask)
RankCase = namedtuple("RankCase", "data chunk_off merges name singles", defaults=(None,))


def well_formed(merges):
    m = [(int(a), int(b)) for a, b in np.asarray(merges).reshape(-1, 2).tolist()]
    return len(set(m)) == len(m) and all(a < 256 + k and b < 256 + k for k, (a, b) in enumerate(m))


def lookup_of(merges):
    return {(int(a), int(b)): 256 + k for k, (a, b) in enumerate(np.asarray(merges).reshape(-1, 2).tolist())}


# ---- the definition, chunk by chunk -------------------------------------------------------------------------------

def _replace(tokens, pair, new):
    out, i = [], 0
    while i < len(tokens):
        if i + 1 < len(tokens) and (tokens[i], tokens[i + 1]) == pair:
            out.append(new)
            i += 2
        else:
            out.append(tokens[i])
            i += 1
    return out


def rank_loop_chunk(tokens, lookup):
    """-> (tokens, number of replacing rounds)"""
    tokens, rounds = list(tokens), 0
    while True:
        ids = [lookup[p] for p in zip(tokens[:-1], tokens[1:]) if p in lookup]
        if not ids:
            return tokens, rounds
        m = min(ids)
        pair = next(p for p in zip(tokens[:-1], tokens[1:]) if lookup.get(p) == m)
        assert all(lookup.get(p) != m or p == pair for p in zip(tokens[:-1], tokens[1:]))
        tokens = _replace(tokens, pair, m)
        rounds += 1


def replay_chunk(tokens, merges):
    tokens = list(tokens)
    for k, (a, b) in enumerate(np.asarray(merges).reshape(-1, 2).tolist()):
        if len(tokens) < 2:
            break
        tokens = _replace(tokens, (int(a), int(b)), 256 + k)
    return tokens


def chunks_of(data, chunk_off):
    data = bytes(data)
    off = [0, len(data)] if chunk_off is None else [int(o) for o in chunk_off]
    return [data[s:e] for s, e in zip(off[:-1], off[1:])]


def rank_loop_chunks(data, chunk_off, merges):
    """-> (tokens of all chunks, token offsets of the chunks, passes: 1 + the most rounds of a chunk; 0 for no text)"""
    lookup = lookup_of(merges)
    out, off, deepest = [], [0], 0
    for ch in chunks_of(data, chunk_off):
        toks, rounds = rank_loop_chunk(text_to_vector(ch), lookup) if ch else ([], 0)
        out += toks
        off.append(len(out))
        deepest = max(deepest, rounds)
    return np.array(out, dtype=np.uint32), np.array(off, dtype=np.uint64), (1 + deepest if len(data) else 0)


def replay_chunks(data, chunk_off, merges):
    out = []
    for ch in chunks_of(data, chunk_off):
        out += replay_chunk(text_to_vector(ch), merges) if ch else []
    return np.array(out, dtype=np.uint32)


# ---- all chunks at once --------------------------------------------------------------------------------------------

def token_stream(data, chunk_off, singles=None):
    """text_to_vector of every chunk -> (tokens uint32, end: True on the last token of a chunk).  singles: ranges that
    are one token whatever their bytes (they are chunks of their own)."""
    data = np.frombuffer(bytes(data), dtype=np.uint8)
    n = len(data)
    off = np.array([0, n], dtype=np.int64) if chunk_off is None else np.asarray(chunk_off).astype(np.int64)
    tok = data.astype(np.uint32)
    end = np.zeros(n, dtype=bool)
    lens = np.diff(off)
    end[off[1:][lens > 0] - 1] = True
    keep = np.ones(n, dtype=bool)
    if singles is None:
        starts = off[:-1][lens > 0]
        for c in np.flatnonzero(data[starts] == 0):
            s = int(starts[c])
            e = int(off[np.searchsorted(off, s, side="right")])
            v = text_to_vector(data[s:e].tobytes())
            if len(v) == 1:                                          # the chunk collapses to one token
                tok[s], end[s] = v[0], True
                keep[s + 1:e] = False
    else:
        for s, ln, i in singles:
            tok[s], end[s] = i, True
            keep[s + 1:s + ln] = False
    return tok[keep], end[keep]


def _take(f):
    """f: candidate mask.  The candidates a left-to-right, non-overlapping walk takes: those that follow an even
    number of consecutive candidates."""
    idx = np.arange(len(f))
    last_false = np.maximum.accumulate(np.where(~f, idx, -1))
    before = np.concatenate([[0], (idx - last_false)[:-1]])          # consecutive candidates right before i
    return f & (before % 2 == 0)


def _apply(tok, end, take, new):
    drop = np.concatenate([[False], take[:-1]])
    tok, end = tok.copy(), end.copy()
    tok[take] = new[take] if isinstance(new, np.ndarray) else new
    at = np.flatnonzero(take)
    end[at] = end[at + 1]
    return tok[~drop], end[~drop]


def rank_loop_text(tok, end, merges):
    """-> (tokens, end, pass_tokens: the tokens that entered every pass, the last of which replaced nothing)"""
    m = np.asarray(merges, dtype=np.uint64).reshape(-1, 2)
    keys = (m[:, 0] << np.uint64(32)) | m[:, 1]
    order = np.argsort(keys, kind="stable")
    keys_sorted, ids_sorted = keys[order], (256 + order).astype(np.uint32)
    last = np.concatenate([keys_sorted[1:] != keys_sorted[:-1], [True]]) if len(keys) else np.zeros(0, dtype=bool)
    keys_sorted, ids_sorted = keys_sorted[last], ids_sorted[last]       # a repeated pair keeps the last id
    pass_tokens = []
    while True:
        pass_tokens.append(len(tok))
        if len(tok) < 2 or len(keys_sorted) == 0:
            return tok, end, pass_tokens
        k = (tok[:-1].astype(np.uint64) << np.uint64(32)) | tok[1:].astype(np.uint64)
        at = np.minimum(np.searchsorted(keys_sorted, k), len(keys_sorted) - 1)
        cand = np.where((keys_sorted[at] == k) & ~end[:-1], ids_sorted[at], np.uint32(NONE))
        cand = np.concatenate([cand, np.array([NONE], dtype=np.uint32)])
        if (cand == NONE).all():
            return tok, end, pass_tokens
        starts = np.concatenate([[0], np.flatnonzero(end)[:-1] + 1]) if end[-1] else \
            np.concatenate([[0], np.flatnonzero(end) + 1])
        seg = np.concatenate([[0], np.cumsum(end)[:-1]])
        low = np.minimum.reduceat(cand, starts)[seg]
        tok, end = _apply(tok, end, _take((cand != NONE) & (cand == low)), cand)


def replay_text(tok, end, merges):
    for k, (a, b) in enumerate(np.asarray(merges).reshape(-1, 2).tolist()):
        if len(tok) < 2:
            break
        f = np.concatenate([(tok[:-1] == a) & (tok[1:] == b) & ~end[:-1], [False]])
        if f.any():
            tok, end = _apply(tok, end, _take(f), np.uint32(256 + k))
    return tok, end


def chunk_tok_off(end, data_len, chunk_off):
    """Token offsets of the chunks from the end flags of the result (an empty chunk repeats its predecessor's)."""
    off = [0, data_len] if chunk_off is None else [int(o) for o in chunk_off]
    ends = np.flatnonzero(end) + 1
    out, k = [0], 0
    for s, e in zip(off[:-1], off[1:]):
        if e > s:
            out.append(int(ends[k]))
            k += 1
        else:
            out.append(out[-1])
    assert k == len(ends)
    return np.array(out, dtype=np.uint64)


def reference(case):
    """-> (tokens, end flags, pass_tokens) of a case in rank order"""
    tok, end = token_stream(case.data, case.chunk_off, case.singles)
    return rank_loop_text(tok, end, case.merges)


# ---- cases --------------------------------------------------------------------------------------------------------

A, B, C, D, Q, X, Y = 97, 98, 99, 100, 113, 120, 121

# (a,b) is the lowest merge; c and d make candidates everywhere (and runs of (c,c), (d,d)); the upper layers keep
# the passes going.  Well-formed.
PLACE_MERGES = np.array([(A, B), (C, D), (D, C), (C, C), (D, D), (256, C), (D, 256), (257, 257), (258, 258), (257, C),
                         (D, 258), (259, 259), (260, 260), (261, 257), (263, 263)], dtype=np.uint32)
CHUNK_LENGTHS = (1, 2, 63, 64, 65, 1023, 1024, 1025, 2049)
MODES = ("first group", "last group", "first span", "last span", "middle span", "several places", "none")


def _background(rng, n):
    return rng.choice(np.array([C, D], dtype=np.uint8), size=n)


def _plant(buf, at):
    if 0 <= at and at + 2 <= len(buf):
        buf[at], buf[at + 1] = A, B


def placement_case(scale=1.0, seed=5):
    """Chunks of CHUNK_LENGTHS tokens that start on, one before and one after a group edge and a span edge (their
    lengths put the ends there too), short chunks of the same alphabet between them; the chunk's one (a,b) -- its
    minimum -- sits where MODES says."""
    span, _, group = E.geometry(scale)
    rng = np.random.default_rng(seed)
    lengths = sorted(set(max(int(round(v * scale)), 1) if scale != 1.0 else v for v in CHUNK_LENGTHS))
    if scale != 1.0:
        lengths = sorted(set([1, 2, group - 1, group, group + 1, span - 1, span, span + 1, 2 * span + 1]))
    parts, n, k = [], 0, 0
    for unit in (group, span):
        for delta in (-1, 0, 1):
            for length in lengths:
                target = (n + 2 + unit - 1) // unit * unit + delta
                while target < n:
                    target += unit
                while n < target:                                    # fillers: chunks of 1 .. 40 bytes
                    ln = min(int(rng.integers(1, 41)), target - n)
                    f = _background(rng, ln)
                    if ln > 3 and rng.integers(0, 3) == 0:
                        _plant(f, int(rng.integers(0, ln - 1)))
                    parts.append(f)
                    n += ln
                buf = _background(rng, length)
                mode = MODES[k % len(MODES)]
                k += 1
                if mode == "first group":
                    _plant(buf, int(rng.integers(0, max(min(group, length) - 1, 1))))
                elif mode == "last group":
                    _plant(buf, length - 2 - int(rng.integers(0, max(min(group, length) - 1, 1))))
                elif mode == "first span":
                    _plant(buf, int(rng.integers(0, max(min(span, length) - 1, 1))))
                elif mode == "last span":
                    _plant(buf, length - 2 - int(rng.integers(0, max(min(span, length) - 1, 1))))
                elif mode == "middle span":
                    _plant(buf, length // 2)
                elif mode == "several places":
                    for at in range(1, length - 1, max(length // 5, 3)):
                        _plant(buf, at)
                parts.append(buf)
                n += length
    data = np.concatenate(parts)
    off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.uint64)
    return RankCase(np.ascontiguousarray(data), off, PLACE_MERGES, "placement: %d chunks, %d bytes" % (len(parts), n))


# (x,y) is lower than the run's pair (a,a): with it in the chunk the run waits a pass
RUN_MERGES = np.array([(X, Y), (A, A), (257, 257), (257, A), (Q, 257)], dtype=np.uint32)


def run_cases(scale=1.0):
    """One chunk each: a run of `a` of length 4 .. 7 that starts 1 .. 3 positions before a group edge / a span edge, q
    around it; `xy` two spans further on, or not at all."""
    span, _, group = E.geometry(scale)
    out = []
    for edge, what in ((3 * group, "group"), (2 * span, "span")):
        for before in (1, 2, 3):
            for length in (4, 5, 6, 7):
                for lower in (True, False):
                    buf = np.full(edge + 2 * span + 10, Q, dtype=np.uint8)
                    buf[edge - before:edge - before + length] = A
                    if lower:
                        buf[edge + 2 * span], buf[edge + 2 * span + 1] = X, Y
                    out.append(RankCase(buf, None, RUN_MERGES, "run: %d a from %d before a %s edge, xy %s" % (
                        length, before, what, "present" if lower else "absent")))
    return out


SLICE_MERGES = PLACE_MERGES[:8]


def slice_cases(scale=1.0, seed=6):
    """2 * slices + 1 spans (per = 3).  One chunk with its only (a,b) in the middle: the minimum crosses the slice
    edges in both directions.  Then two chunks that meet exactly at a slice edge, the (a,b) at the far end of one of
    them: it travels the whole chunk and stops at the edge."""
    span, slices, _ = E.geometry(scale)
    rng = np.random.default_rng(seed)
    n_spans = 2 * slices + 1
    n = (n_spans - 1) * span + span // 2 + 1
    per = -(-n_spans // slices)
    assert per == 3
    cut = (slices // 3) * per * span
    out = []
    for name, off, at in (("one chunk, (a,b) in the middle", None, n // 2),
                          ("cut at a slice edge, (a,b) at the start of the first chunk", [0, cut, n], 0),
                          ("cut at a slice edge, (a,b) at the end of the second chunk", [0, cut, n], n - 2)):
        buf = _background(rng, n)
        _plant(buf, at)
        out.append(RankCase(buf, None if off is None else np.array(off, dtype=np.uint64), SLICE_MERGES,
                            "slices: %s, %d spans" % (name, n_spans)))
    return out


SPECIAL_IDS = (300, 70000, 7)
# pairs of a special id with its neighbours' bytes: a merge across a chunk end would show
SPECIAL_MERGES = np.concatenate([PLACE_MERGES, np.array(
    [(i, c) for i in SPECIAL_IDS for c in (C, D, A)] + [(c, i) for i in SPECIAL_IDS for c in (C, D, B)] +
    [(i, j) for i in SPECIAL_IDS for j in SPECIAL_IDS] + [(0, 51), (51, 48), (48, 48)], dtype=np.uint32)])


def special_case(scale=1.0, seed=8, as_singles=False):
    """Single-token chunks directly before and after chunks of several groups (and two in a row).  as_singles: the
    ranges are given by position, as mbpe_encoder_encode_endmask takes them, and their bytes are ordinary text;
    otherwise they are the chunks NUL + decimal id."""
    span, _, group = E.geometry(scale)
    rng = np.random.default_rng(seed)
    parts, singles, n = [], [], 0
    k = 0
    for length in (3 * group + 5, 1, 2 * group, span + group + 1, 2, group, 2 * span + 3):
        for _ in range(1 + (k % 3 == 1)):
            i = SPECIAL_IDS[k % len(SPECIAL_IDS)]
            k += 1
            marker = np.frombuffer(b"cdab"[:1 + k % 4] if as_singles else b"\0%d" % i, dtype=np.uint8)
            singles.append((n, len(marker), i))
            parts.append(marker)
            n += len(marker)
        buf = _background(rng, length)
        _plant(buf, length // 2)
        parts.append(buf)
        n += length
    i = SPECIAL_IDS[0]
    marker = np.frombuffer(b"dc" if as_singles else b"\0%d" % i, dtype=np.uint8)
    singles.append((n, len(marker), i))
    parts.append(marker)
    data = np.ascontiguousarray(np.concatenate(parts))
    off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.uint64)
    return RankCase(data, off, SPECIAL_MERGES, "specials%s: %d chunks" % (" as singles" * as_singles, len(parts)),
                    singles if as_singles else None)


def random_merges(rng, n_merges, alphabet):
    """A well-formed table: every side below its own id, no pair twice; low ids are favoured, so that deep tokens
    actually occur in a random text."""
    seen, out = set(), []
    while len(out) < n_merges:
        hi = len(out)
        pick = []
        for _ in range(2):
            if hi and rng.integers(0, 3):
                pick.append(256 + int(rng.integers(0, hi if rng.integers(0, 2) else min(hi, 30))))
            else:
                pick.append(int(alphabet[int(rng.integers(0, len(alphabet)))]))
        p = tuple(pick)
        if p not in seen:
            seen.add(p)
            out.append(p)
    return np.array(out, dtype=np.uint32)


def fuzz_case(seed, n_bytes=300000, max_merges=1744):
    rng = np.random.default_rng(seed)
    alphabet = np.arange(97, 97 + int(rng.integers(2, 8)), dtype=np.uint8)
    merges = random_merges(rng, int(rng.integers(5, max_merges + 1)), alphabet)
    data = rng.choice(alphabet, size=n_bytes)
    if rng.integers(0, 2):                                            # runs
        data = np.repeat(data[:n_bytes // 4 + 1], rng.integers(1, 9, size=n_bytes // 4 + 1))[:n_bytes]
    mean = int(rng.choice([3, 8, 40, 700, 5000]))
    cuts = np.unique(rng.integers(1, n_bytes, size=max(n_bytes // mean, 1)))
    off = np.concatenate([[0], cuts, [n_bytes]]).astype(np.uint64)
    assert well_formed(merges)
    return RankCase(np.ascontiguousarray(data), off, merges, "fuzz %d: %d bytes, alphabet %d, %d merges, %d chunks" % (
        seed, n_bytes, len(alphabet), len(merges), len(off) - 1))


# tables for which only the loop is the definition
REPEATED_PAIR = np.array([(A, B), (B, C), (A, B)], dtype=np.uint32)          # (a,b) keeps the last id, 258
HIGH_SIDE = np.array([(257, C), (A, B)], dtype=np.uint32)                     # merge 0 needs the token of merge 1
