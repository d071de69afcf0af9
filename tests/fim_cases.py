"""The fill-in-the-middle rule (include/mbpe.h, mbpe_fim_spec) restated in Python: what mbpe_fim_plan,
mbpe_fim_tokens and the encoder's stage are held to, and the case lists of the CPU and GPU tests."""
import numpy as np

M64 = (1 << 64) - 1
ONE = 1 << 32                       # the threshold of probability 1
NONE, PSM, SPM = 0, 1, 2
PRE, SUF, MID = 60001, 60002, 60003


def ref_hash(seed, pos, idx):
    """csrc/dropout.h, drop_hash: one round of splitmix64's finisher over a linear mix; the high 32 bits."""
    x = (seed + pos * 0x9E3779B97F4A7C15 + idx * 0xD1B54A32D192ED03) & M64
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & M64
    x ^= x >> 31
    return x >> 32


def spec(rate=ONE, spm=ONE // 2, seed=0, doc_base=0, pre=PRE, suf=SUF, mid=MID, min_tokens=0, max_tokens=0):
    """The rule's parameters as a dict; rate and spm are thresholds in [0, 2^32]."""
    return dict(rate=rate, spm=spm, seed=seed, doc_base=doc_base, pre=pre, suf=suf, mid=mid, min_tokens=min_tokens,
                max_tokens=max_tokens)


def threshold(p):
    return int(p * 4294967296.0)


def ref_plan_doc(s, d, L):
    """(mode, a, b) of document d of the call, L tokens long; (NONE, 0, 0) where it stays as it is."""
    g = (s["doc_base"] + d) & M64
    if L < max(s["min_tokens"], 1) or (s["max_tokens"] != 0 and L > s["max_tokens"]):
        return NONE, 0, 0
    if ref_hash(s["seed"], g, 0) >= s["rate"]:
        return NONE, 0, 0
    c1 = (ref_hash(s["seed"], g, 1) * (L + 1)) >> 32
    c2 = (ref_hash(s["seed"], g, 2) * (L + 1)) >> 32
    mode = SPM if ref_hash(s["seed"], g, 3) < s["spm"] else PSM
    return mode, min(c1, c2), max(c1, c2)


def ref_plan(lens, s):
    """-> (offsets after the transform [n + 1], modes [n], cuts [n][2])."""
    off, modes, cuts = [0], [], []
    for d, L in enumerate(lens):
        mode, a, b = ref_plan_doc(s, d, L)
        modes.append(mode)
        cuts.append([a, b])
        off.append(off[-1] + L + (3 if mode else 0))
    return off, modes, cuts


def ref_apply_doc(t, mode, a, b, s):
    t = list(t)
    P, M, S = t[:a], t[a:b], t[b:]
    if mode == PSM:
        return [s["pre"]] + P + [s["suf"]] + S + [s["mid"]] + M
    if mode == SPM:
        return [s["pre"], s["suf"]] + S + [s["mid"]] + P + M
    return t


def ref_apply(docs, s):
    """The transform of a list of token lists -> the list of the new token lists."""
    return [ref_apply_doc(t, *ref_plan_doc(s, d, len(t)), s) for d, t in enumerate(docs)]


def ref_unapply_doc(t, mode, a, b):
    """The inverse for a known plan (the new list has len + 3 ids)."""
    t = list(t)
    if mode == NONE:
        return t
    L = len(t) - 3
    ns = L - b
    if mode == PSM:
        return t[1:1 + a] + t[3 + a + ns:] + t[2 + a:2 + a + ns]
    return t[3 + ns:] + t[2:2 + ns]


def ref_unapply(new_docs, lens, s):
    return [ref_unapply_doc(t, *ref_plan_doc(s, d, L)) for d, (t, L) in enumerate(zip(new_docs, lens))]


def flat(docs, dtype=np.uint32):
    """(flat token array, offsets uint64[n + 1]) of a list of token lists."""
    off = np.zeros(len(docs) + 1, dtype=np.uint64)
    if docs:
        off[1:] = np.cumsum([len(t) for t in docs], dtype=np.uint64)
    tok = np.array([v for t in docs for v in t], dtype=dtype)
    return tok, off


def docs_of_lens(lens, rng, hi=60000):
    return [[rng.randrange(0, hi) for _ in range(L)] for L in lens]


def grid_lens(n_docs):
    """Document lengths 0 .. 40 in a fixed order that is no multiple of the wave or the span."""
    return [(7 * i + i // 41) % 41 for i in range(n_docs)]


# the grid of the CPU test
GRID_N_DOCS = [0, 1, 2, 1023, 1024, 1025, 2049]
GRID_RATES = [0.0, 0.5, 1.0]
GRID_LIMITS = [(0, 0), (5, 0), (0, 30), (5, 30)]                # (min_tokens, max_tokens)
GRID_BASES = [0, 1 << 40]

# one batch whose cuts fall into different pieces and spans
MIXED_LENS = [0, 1, 2, 3, 5, 64, 1023, 1024, 1025, 5000, 0, 7]
