"""BPE-dropout in rank order (mbpe_encoder_set_dropout, Tokenizer.encode(order="rank", dropout=p, seed=s)): a
pure-Python / numpy reference and case generators.  No GPU, no product code.

The definition (include/mbpe.h), per chunk, after text_to_vector, repeat: of the adjacent pairs (t[i], t[i + 1]) that
are in the lookup AND whose instance is not dropped take the smallest merged id m; stop if there is none; replace the
surviving instances of m, left to right and non-overlapping.  An instance is (pos, id): pos = the offset of the first
byte of t[i] in the buffer the encoder read, id = the merged token; it is dropped iff drop_hash(seed, pos, id) <
threshold.  Restatements:
  drop_hash           on Python integers; drop_hash_np the same on numpy arrays
  dropout_loop_chunk  the loop as written above on Python lists that carry the byte starts (small inputs)
  dropout_loop_text   the loop over all chunks of a text at once, in numpy, modelled on encode_rank_cases.rank_loop_text;
                      it carries the byte starts, which are also the token byte offsets the _byteoff calls report
"""
import numpy as np

import encode_rank_cases as R
from test_bruteforce_cpu import text_to_vector

NONE = 0xFFFFFFFF
M64 = (1 << 64) - 1
ONE = 1 << 32                                   # the threshold of p = 1

# (seed, pos, id) -> drop_hash: the known answers of the definition
KNOWN = [(0, 0, 256, 0xa4a47e7e), (0, 1, 256, 0x57cb3d0c), (1, 0, 256, 0x926993ad), (42, 1023, 511, 0xcac74bc6),
         ((1 << 64) - 1, (1 << 40) + 5, 65535, 0x59525672), (7, 1 << 32, 16777215, 0xf3b38aaa)]


def drop_hash(seed, pos, idx):
    x = (seed + pos * 0x9E3779B97F4A7C15 + idx * 0xD1B54A32D192ED03) & M64
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & M64
    x ^= x >> 31
    return x >> 32


def dropped(seed, pos, idx, threshold):
    return drop_hash(seed, pos, idx) < threshold


def threshold_of(p):
    """floor(p * 2^32); p * 2^32 is exact in a double, so int() is the floor"""
    assert 0.0 <= p <= 1.0
    return int(p * 4294967296.0)


def drop_hash_np(seed, pos, idx):
    """pos, idx: arrays -> uint64 array of the 32-bit hashes (uint64 arithmetic wraps mod 2^64)"""
    with np.errstate(over="ignore"):
        x = np.uint64(seed & M64) + np.asarray(pos, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + \
            np.asarray(idx, dtype=np.uint64) * np.uint64(0xD1B54A32D192ED03)
        x ^= x >> np.uint64(30)
        x *= np.uint64(0xBF58476D1CE4E5B9)
        x ^= x >> np.uint64(27)
        x *= np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(31)
    return x >> np.uint64(32)


# ---- the definition, chunk by chunk ----------------------------------------------------------------------------------

def dropout_loop_chunk(tokens, lookup, base, seed, threshold):
    """tokens: text_to_vector of a chunk whose first byte is at `base` -> (tokens, byte starts, replacing rounds)"""
    tokens = list(tokens)
    pos = [base + i for i in range(len(tokens))]
    rounds = 0
    while True:
        cand = []
        for i in range(len(tokens) - 1):
            m = lookup.get((tokens[i], tokens[i + 1]))
            cand.append(None if m is None or dropped(seed, pos[i], m, threshold) else m)
        live = [m for m in cand if m is not None]
        if not live:
            return tokens, pos, rounds
        low = min(live)
        out, out_pos, i = [], [], 0
        while i < len(tokens):
            hit = i + 1 < len(tokens) and cand[i] == low
            out.append(low if hit else tokens[i])
            out_pos.append(pos[i])
            i += 2 if hit else 1
        tokens, pos = out, out_pos
        rounds += 1


def dropout_loop_chunks(data, chunk_off, merges, seed, threshold):
    """-> (tokens of all chunks, their byte starts, token offsets of the chunks, passes: 1 + the most rounds)"""
    lookup = R.lookup_of(merges)
    data = bytes(data)
    off = [0, len(data)] if chunk_off is None else [int(o) for o in chunk_off]
    out, starts, tok_off, deepest = [], [], [0], 0
    for s, e in zip(off[:-1], off[1:]):
        if e > s:
            toks, pos, rounds = dropout_loop_chunk(text_to_vector(data[s:e]), lookup, s, seed, threshold)
            out += toks
            starts += pos
            deepest = max(deepest, rounds)
        tok_off.append(len(out))
    return (np.array(out, dtype=np.uint32), np.array(starts, dtype=np.uint64), np.array(tok_off, dtype=np.uint64),
            1 + deepest if len(data) else 0)


# ---- all chunks at once ------------------------------------------------------------------------------------------------

def token_stream(data, chunk_off, singles=None):
    """encode_rank_cases.token_stream with the byte start of every token -> (tokens, end, pos)"""
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
            if len(v) == 1:
                tok[s], end[s] = v[0], True
                keep[s + 1:e] = False
    else:
        for s, ln, i in singles:
            tok[s], end[s] = i, True
            keep[s + 1:s + ln] = False
    return tok[keep], end[keep], np.arange(n, dtype=np.uint64)[keep]


def dropout_loop_text(tok, end, pos, merges, seed, threshold):
    """-> (tokens, end, pos, pass_tokens: the tokens that entered every pass, the last of which replaced nothing)"""
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
            return tok, end, pos, pass_tokens
        k = (tok[:-1].astype(np.uint64) << np.uint64(32)) | tok[1:].astype(np.uint64)
        at = np.minimum(np.searchsorted(keys_sorted, k), len(keys_sorted) - 1)
        cand = np.where((keys_sorted[at] == k) & ~end[:-1], ids_sorted[at], np.uint32(NONE))
        hit = cand != NONE
        gone = np.zeros(len(cand), dtype=bool)
        gone[hit] = drop_hash_np(seed, pos[:-1][hit], cand[hit]) < np.uint64(threshold)
        cand = np.concatenate([np.where(gone, np.uint32(NONE), cand), np.array([NONE], dtype=np.uint32)])
        if (cand == NONE).all():
            return tok, end, pos, pass_tokens
        starts = np.concatenate([[0], np.flatnonzero(end)[:-1] + 1]) if end[-1] else \
            np.concatenate([[0], np.flatnonzero(end) + 1])
        seg = np.concatenate([[0], np.cumsum(end)[:-1]])
        low = np.minimum.reduceat(cand, starts)[seg]
        take = R._take((cand != NONE) & (cand == low))
        swallowed = np.concatenate([[False], take[:-1]])
        tok, end = R._apply(tok, end, take, cand)
        pos = pos[~swallowed]                                          # a merged token keeps its left token's start


def reference(data, chunk_off, merges, seed, threshold, singles=None):
    """-> (tokens, end flags, byte starts, pass_tokens)"""
    return dropout_loop_text(*token_stream(data, chunk_off, singles), merges, seed, threshold)


def byte_offsets(pos, n_bytes):
    """the n + 1 token byte offsets of a text the chunks tile: every token's start, then the end of the text"""
    return np.concatenate([pos, [n_bytes]]).astype(np.uint64)


# ---- cases -------------------------------------------------------------------------------------------------------------

A, B = 97, 98
TINY_MERGES = np.array([(A, A), (256, 256), (A, B), (258, 258)], dtype=np.uint32)
TINY_LENGTHS = (0, 1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 2049)
TINY_THRESHOLDS = (0, 1 << 31, ONE)
TINY_SEEDS = (0, 0xDEADBEEFCAFEF00D)


def tiny_text(kind, n):
    return (b"a" * n) if kind == "a" else (b"ab" * (n // 2 + 1))[:n]


def tiny_chunkings(n):
    """one chunk; chunks that end at 63 / 64 / 65; chunks that end at 1,023 / 1,024 / 1,025 -> lists of offsets"""
    out = [None]
    for cuts in ((63, 64, 65), (1023, 1024, 1025)):
        off = [0] + [c for c in cuts if c < n] + [n]
        if len(off) > 2:
            out.append(np.array(off, dtype=np.uint64))
    return out


# ten nested merges, two ways.  A chain over the word a..k: level k adds one letter, so a whole word needs all ten of its
# instances to survive -- at p = 0.1 a third of the words do, and the encode still takes one pass per level while the
# stream shrinks from 4,096 tokens to a few hundred and tokens cross span edges.  And a doubling over one letter: a
# 4,096-byte run halves per pass without dropout; with it the survivors of every level sit at hash-chosen places and the
# left-to-right rule runs over what is left of the runs
NESTED_WORD = b"abcdefghijk"
NESTED_MERGES = np.array([(A, B)] + [(255 + k, A + 1 + k) for k in range(1, 10)], dtype=np.uint32)
DOUBLING_MERGES = np.array([(A, A)] + [(255 + k, 255 + k) for k in range(1, 10)], dtype=np.uint32)


def nested_chunk():
    return (NESTED_WORD * (4096 // len(NESTED_WORD) + 1))[:4096]


def doubling_chunk():
    return b"a" * 4096


def many_chunk_text(n_bytes=5000, seed=11, n_merges=40):
    """random text over a small alphabet, cut into chunks of 1 .. 60 bytes, with a random well-formed table"""
    rng = np.random.default_rng(seed)
    alphabet = np.arange(97, 101, dtype=np.uint8)
    merges = R.random_merges(rng, n_merges, alphabet)
    data = rng.choice(alphabet, size=n_bytes)
    cuts, at = [0], 0
    while at < n_bytes:
        at = min(at + int(rng.integers(1, 61)), n_bytes)
        cuts.append(at)
    return np.ascontiguousarray(data).tobytes(), np.array(cuts, dtype=np.uint64), merges


def generated_strings(seed=3, n=200):
    """short strings over {a, b, c} with a table of runs and nested pairs, for the literal loops"""
    rng = np.random.default_rng(seed)
    merges = np.array([(A, A), (A, B), (256, 256), (257, 99), (256, A), (98, 98), (261, 261)], dtype=np.uint32)
    out = []
    for _ in range(n):
        ln = int(rng.integers(0, 40))
        out.append(bytes(rng.choice(np.array([97, 97, 97, 98, 99], dtype=np.uint8), size=ln).tolist()))
    return out, merges
