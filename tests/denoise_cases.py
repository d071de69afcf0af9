"""The span-corruption rule (include/mbpe.h, mbpe_denoise_spec) restated in Python: what mbpe_denoise_plan,
mbpe_denoise_tokens and the encoder's denoise calls are held to, and the case lists of the CPU and GPU tests."""
import numpy as np

from fim_cases import ref_hash

M64 = (1 << 64) - 1
ONE = 1 << 32                       # the threshold of density 1
SENT = 32099                        # T5's <extra_id_0>
T5_DENSITY = int(0.15 * 2 ** 32)


def spec(density=T5_DENSITY, mean_q8=768, seed=0, doc_base=0, seg=0, min_tokens=0, sent=SENT, down=1, n_sent=100):
    """The rule's parameters as a dict; density is a threshold in [0, 2^32], mean_q8 the mean part length in 1/256."""
    return dict(density=density, mean_q8=mean_q8, seed=seed, doc_base=doc_base, seg=seg, min_tokens=min_tokens,
                sent=sent, down=down, n_sent=n_sent)


def threshold(p):
    return int(p * 4294967296.0)


# ---- the restatement, as the issue gives it ---------------------------------------------------------------------------

def counts(s, L):
    if s["density"] == 0 or L < max(s["min_tokens"], 2):
        return 0, 0
    N = min(max((L * s["density"] + (1 << 31)) >> 32, 1), L - 1)
    S = (N * 256 + s["mean_q8"] // 2) // s["mean_q8"]
    return N, max(1, min(S, N, L - N, s["n_sent"]))


def bounds(su, T, S, c):
    E = T - S
    q = lambda j: (j * E) // S
    cs = [0] + [q(j - 1) + ((ref_hash(su, j, c) * (q(j) - q(j - 1) + 1)) >> 32) for j in range(1, S)] + [E]
    return [j + cs[j] for j in range(S + 1)]


def unit_seed(s, d, u):
    g = (s["doc_base"] + d) & M64
    sg = (ref_hash(s["seed"], g, 0x44454E00) << 32) | ref_hash(s["seed"], g, 0x44454E01)
    return (ref_hash(sg, u, 2) << 32) | ref_hash(sg, u, 3)


def sid(s, j):
    return s["sent"] - j if s["down"] else s["sent"] + j


def ref_unit(s, d, u, t):
    t = list(t)
    L = len(t)
    N, S = counts(s, L)
    if S == 0:
        return list(t), []
    su = unit_seed(s, d, u)
    Bn = bounds(su, N, S, 0)
    Bm = bounds(su, L - N, S, 1)
    inp, tg, p = [], [], 0
    for j in range(S):
        m, n = Bm[j + 1] - Bm[j], Bn[j + 1] - Bn[j]
        inp += t[p:p + m] + [sid(s, j)]
        p += m
        tg += [sid(s, j)] + t[p:p + n]
        p += n
    return inp, tg


# ---- the closed forms a gather may use --------------------------------------------------------------------------------

def ref_input_at(s, d, u, t, p):
    """The id at position p of the unit's inputs, by the closed form alone."""
    L = len(t)
    N, S = counts(s, L)
    if S == 0:
        return t[p]
    su = unit_seed(s, d, u)
    Bn, Bm = bounds(su, N, S, 0), bounds(su, L - N, S, 1)
    j = min(j for j in range(S) if Bm[j + 1] + j >= p)
    return sid(s, j) if Bm[j + 1] + j == p else t[p - j + Bn[j]]


def ref_target_at(s, d, u, t, p):
    L = len(t)
    N, S = counts(s, L)
    su = unit_seed(s, d, u)
    Bn, Bm = bounds(su, N, S, 0), bounds(su, L - N, S, 1)
    j = max(j for j in range(S) if Bn[j] + j <= p)
    return sid(s, j) if Bn[j] + j == p else t[p - j - 1 + Bm[j + 1]]


# ---- documents -> units -> the two streams ----------------------------------------------------------------------------

def units_of(s, L):
    """[(first token, length)] of the units of a document of L tokens."""
    seg = s["seg"]
    if seg == 0 or L <= seg:
        return [(0, L)]
    return [(a, min(seg, L - a)) for a in range(0, L, seg)]


def ref_apply(docs, s):
    """docs: lists of ids -> (inputs per unit, targets per unit, unit_doc)."""
    ins, tgs, unit_doc = [], [], []
    for d, t in enumerate(docs):
        for u, (a, n) in enumerate(units_of(s, len(t))):
            i, g = ref_unit(s, d, u, list(t[a:a + n]))
            ins.append(i)
            tgs.append(g)
            unit_doc.append(d)
    return ins, tgs, unit_doc


def ref_plan(lens, s):
    """-> (unit_in_off, unit_tg_off, unit_doc) from the counts alone."""
    in_off, tg_off, unit_doc = [0], [0], []
    for d, L in enumerate(lens):
        for _, n in units_of(s, L):
            N, S = counts(s, n)
            in_off.append(in_off[-1] + n - N + S)
            tg_off.append(tg_off[-1] + (N + S if S else 0))
            unit_doc.append(d)
    return in_off, tg_off, unit_doc


def flat(rows, dtype=np.uint32):
    """Lists of ids -> (flat array, offsets)."""
    off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint64)
    out = np.array([x for r in rows for x in r], dtype=dtype) if off[-1] else np.zeros(0, dtype=dtype)
    return out, off


def docs_of_lens(lens, rng, vocab=30000):
    """Documents of these lengths with distinct-looking ids below the sentinels."""
    return [[rng.randrange(vocab) for _ in range(L)] for L in lens]


# ---- the grid of the CPU tests ------------------------------------------------------------------------------------------

GRID_LENS = list(range(40)) + [511, 512, 568, 1025, 5000]
GRID_DENSITIES = (0.0, 0.15, 0.5, 1.0)
GRID_SHAPES = ((768, 100), (256, 100), (768, 2), (1280, 1))       # (mean_q8, n_sentinels)
