"""The weighted 32-bit training loop at its limits -- a pair count of 2^31 is refused, a sum of counts beyond 2^32 is not
-- as cases of a few thousand tokens: the generators and the reference of tests/test_weighted_limits_cpu.py and of the GPU
tests (test_gpu_weighted_limits.py, test_gpu_weighted_limits_pieces.py).  The reference is dedup_cases.weighted_bpe, which
works on Python integers and so has no 32-bit limit.  A case is (chunks, weights, vocab, expect); expect is "trains" iff
every weighted pair count of the corpus is below L = 2^31 (later counts never exceed an earlier chosen one), else
"overflow".  Needs neither a GPU nor torch."""
import collections
import functools

import numpy as np

import dedup_cases as C

L = 1 << 31
SHARE = 4096            # the least a workgroup of the pair count takes (launch_wide_pair_count_tokens)
SPAN = 1024             # tokens per wave of the loop's span kernels
LDS_SLOTS = 1024        # pairs a workgroup of the pair count caches; the rest goes to the table directly
LDS_PROBES = 4          # slots it tries for a pair before it does
VOCAB = 256 + 40
SMALL_VOCAB = 256 + 12
N_PRIOR = 10

Reference = collections.namedtuple("Reference", "merges counts seqs table")


# ---- the reference -------------------------------------------------------------------------------------------------
def pair_positions(seqs):
    """(position in the stream, pair) of every pair of the token sequences, in stream order."""
    p = 0
    for s in seqs:
        for i in range(len(s) - 1):
            yield p + i, (s[i], s[i + 1])
        p += len(s)


def recount(seqs, weights):
    """The weighted pair table of token sequences, in Python integers (no zero entries)."""
    tab = {}
    for s, w in zip(seqs, weights):
        for i in range(len(s) - 1):
            key = (s[i], s[i + 1])
            tab[key] = tab.get(key, 0) + w
    return tab


def initial_counts(chunks, weights):
    return recount(chunks, weights)


def replay(chunks, prior):
    """The chunks as token sequences after the prior merges, each applied to the whole text in rank order."""
    seqs = [list(c) for c in chunks]
    for k, (a, b) in enumerate(prior):
        for n, s in enumerate(seqs):
            out, i = [], 0
            while i < len(s):
                if i + 1 < len(s) and s[i] == a and s[i + 1] == b:
                    out.append(256 + k)
                    i += 2
                else:
                    out.append(s[i])
                    i += 1
            seqs[n] = out
    return seqs


def reference(chunks, weights, vocab, first_mode, prior=None):
    """-> Reference: the merges and counts made (after the prior ones), the final token sequences, and the final non-zero
    pair table recounted with weights from those sequences."""
    weights = [int(w) for w in weights]
    start = None if prior is None else (replay(chunks, [tuple(int(x) for x in p) for p in prior]), len(prior))
    merges, counts, seqs = C.weighted_bpe(chunks, weights, vocab, first_mode, start=start, with_seqs=True)
    return Reference(merges, counts, seqs, recount(seqs, weights))


# ---- what the launcher does with a stream ------------------------------------------------------------------------------
def n_tokens(chunks):
    return sum(len(c) for c in chunks)


def shares(n_tok, n_cus=256):
    """The [lo, hi) token ranges of the pair count's workgroups (launch_wide_pair_count_tokens)."""
    if n_tok < 2:
        return []
    blocks = min(n_cus * 8, (n_tok + SHARE - 1) // SHARE)
    blocks = max(blocks, (n_tok + (1 << 20) - 1) >> 20)
    per = (n_tok + blocks - 1) // blocks
    return [(b * per, min(b * per + per, n_tok)) for b in range(blocks) if b * per < n_tok]


def n_spans(chunks):
    return (n_tokens(chunks) + SPAN - 1) // SPAN


def positions_of(chunks, pair):
    return [p for p, key in pair_positions(chunks) if key == pair]


def distinct_pairs(chunks, lo, hi):
    """The distinct pairs that start at the stream positions lo .. hi - 1."""
    return {key for p, key in pair_positions(chunks) if lo <= p < hi}


# ---- generators ----------------------------------------------------------------------------------------------------------
def scale_weights(chunks, raw, target):
    """raw weights divided by one common factor, the smallest for which no pair count exceeds `target`."""
    top = max(initial_counts(chunks, raw).values())
    factor = (top + target - 1) // target
    return [min(max(1, int(r) // factor), L - 1) for r in raw]


def random_weights(seed, n):
    rng = np.random.default_rng(seed)
    return [int(x) for x in rng.integers(1, 1 << 41, size=n)]


def _fill(seed, total, n_sym, base, max_len):
    """Chunks of 1 .. max_len bytes over n_sym symbols from `base`, of exactly `total` bytes together."""
    rng = np.random.default_rng(seed)
    out, left = [], total
    while left > 0:
        n = min(int(rng.integers(1, max_len + 1)), left)
        out.append(bytes(rng.integers(base, base + n_sym, size=n, dtype=np.uint8)))
        left -= n
    return out


def _place(filler, filler_weights, heavy, at):
    """filler with the (chunk, weight) of heavy[i] put in at the first chunk boundary at or after token at[i]."""
    chunks, weights = [], []
    todo = sorted(zip(at, range(len(heavy))))
    pos = 0
    for c, w in zip(filler, filler_weights):
        while todo and todo[0][0] <= pos:
            h = heavy[todo.pop(0)[1]]
            chunks.append(h[0])
            weights.append(h[1])
            pos += len(h[0])
        chunks.append(c)
        weights.append(w)
        pos += len(c)
    for _, i in todo:
        chunks.append(heavy[i][0])
        weights.append(heavy[i][1])
    return chunks, weights


def _case(chunks, weights, vocab):
    expect = "trains" if max(initial_counts(chunks, weights).values()) < L else "overflow"
    return chunks, weights, vocab, expect


@functools.lru_cache(maxsize=None)
def sum_beyond_2_32(variant):
    """About 2,300 distinct chunks over 24 symbols whose weighted positions add up to far more than 2^32 while the top
    count stays just below L.  "a": one weight for all; "b": independent weights."""
    chunks = list(dict.fromkeys(C.random_chunks(3, 2500, 12, 24)))
    if variant == "a":
        top_unit = max(initial_counts(chunks, [1] * len(chunks)).values())
        weights = [(L - 1) // top_unit] * len(chunks)
    else:
        weights = scale_weights(chunks, random_weights(32, len(chunks)), L - 1)
    return _case(chunks, weights, VOCAB)


@functools.lru_cache(maxsize=None)
def many_distinct_pairs():
    """64 symbols: a share of 4,096 tokens holds well over 1,024 distinct pairs, so that most of them are added to the
    table directly, each with a large weight of its own."""
    chunks = list(dict.fromkeys(_fill(64, 8000, 64, 48, 24)))
    weights = scale_weights(chunks, random_weights(65, len(chunks)), L - 1)
    return _case(chunks, weights, VOCAB)


LADDER_COUNTS = [L - 2, L - 1, L, L + 1, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, 3 * L, (1 << 33) + 5]
LAYOUTS = ["one_share", "in_chunk", "in_run", "across_shares", "direct"]
A, B = 33, 34           # the heavy pair: '!', '"' -- small byte values, below every filler symbol


def lds_slot(pair):
    """The first of the LDS_PROBES consecutive cache slots k_wide_pair_count_tokens tries for a pair (pair_hash, span.h)."""
    key = (pair[0] << 32) | pair[1]
    return ((key * 0x9E3779B97F4A7C15) & ((1 << 64) - 1)) >> 54


def cache_is_full_for(chunks, pair, lo, before):
    """Whether each cache slot `pair` may take is the first choice of some other pair that starts in lo .. before - 1: a
    slot that is someone's first choice is taken from then on, by that pair or by an earlier one, so that an occurrence
    of `pair` counted after all of those positions finds no entry and goes to the table directly."""
    taken = {lds_slot(key) for p, key in pair_positions(chunks) if lo <= p < before and key != pair}
    return all((lds_slot(pair) + i) % LDS_SLOTS in taken for i in range(LDS_PROBES))


def _direct_filler():
    return list(dict.fromkeys(_fill(9, 8000, 64, 48, 24)))


@functools.lru_cache(maxsize=None)
def _direct_pair():
    """The heavy pair of the "direct" layout: the first pair of small byte values whose cache slots the filler has taken
    long before the pair shows, in either share."""
    filler = _direct_filler()
    for a in range(A, 48):
        for b in range(a + 1, 48):
            if cache_is_full_for(filler, (a, b), 0, 1900) and cache_is_full_for(filler, (a, b), 4100, 5900):
                return a, b
    raise AssertionError("no pair found")


def heavy_pair(layout):
    return (A, A) if layout == "in_run" else _direct_pair() if layout == "direct" else (A, B)


def _heavy_chunks(c, layout):
    """(chunk, weight) of the chunks that hold the heavy pair: their weights are below L, the pair's count is exactly c,
    and no other pair of theirs reaches 2^30."""
    a, b = heavy_pair(layout)
    ab = bytes([a, b])
    fixed = []                                  # (chunk, weight, occurrences in the chunk)
    if layout == "in_chunk":                    # `abab`: touching candidates, and (b, a) beside them
        fixed = [(ab * 2, (1 << 27) + 1, 2), (ab * 3, (1 << 27) + 3, 3), (b"k" + ab * 2 + b"l", (1 << 26) + 5, 2)]
    elif layout == "in_run":                    # `aaa`: overlapping positions, every second one a match
        fixed = [(bytes([a] * 3), (1 << 28) + 1, 2), (bytes([a] * 4), (1 << 27) + 3, 3),
                 (b"k" + bytes([a] * 5) + b"l", (1 << 26) + 5, 4)]
    rest = c - sum(w * occ for _, w, occ in fixed)
    around = [(b"m", b""), (b"", b"n"), (b"o", b"p"), (b"q", b""), (b"", b"r"), (b"s", b"t"), (b"u", b""), (b"", b"v")]
    for m in range(3, len(around) + 1):         # m chunks with neighbours (below 2^30 each) and the bare pair
        per = min((1 << 30) - 1, rest // (m + 1))
        with_neighbours = [per - i for i in range(m)]
        bare = rest - sum(with_neighbours)
        if bare < L:
            break
    assert 0 < bare < L and min(with_neighbours) > 0
    out = [(x + ab + y, w) for (x, y), w in zip(around, with_neighbours)]
    out.insert(1, (ab, bare))
    out[2:2] = [(ch, w) for ch, w, _ in fixed]
    assert sum(w * len(positions_of([ch], (a, b))) for ch, w in out) == c
    return out


@functools.lru_cache(maxsize=None)
def ladder(c, layout):
    """One pair whose count is exactly c, from several chunks with weights below L; every other count is below 2^30.
    "one_share": all of it within one workgroup's share of the pair count (its LDS counter); "in_chunk", "in_run":
    also from several occurrences within a chunk; "across_shares": from at least three shares, filler of weight 1
    between them (the table's own sum); "direct": late in shares that hold more pairs than the LDS cache, a pair for
    which the cache has no slot left by then."""
    heavy = _heavy_chunks(c, layout)
    k = len(heavy)
    if layout == "across_shares":
        filler = _fill(7, 13000, 24, 97, 12)
        fw = [1] * len(filler)
        at = [(2 * i + 1) * 13000 // (2 * k) for i in range(k)]
    elif layout == "direct":
        filler = _direct_filler()
        fw = scale_weights(filler, random_weights(10, len(filler)), (1 << 30) - 1)
        # late in either share, where the cache is full: for this pair in particular (_direct_pair)
        at = [3000 + 150 * i if i % 2 == 0 else 7000 + 100 * i for i in range(k)]
    else:
        filler = _fill(5, 1500, 24, 97, 12)
        fw = [1] * len(filler)
        at = [150 + 10 * i if i % 2 == 0 else 1100 + 10 * i for i in range(k)]
    chunks, weights = _place(filler, fw, heavy, at)
    return _case(chunks, weights, SMALL_VOCAB)


TIED = [(A, B), (35, 36), (122, 121)]          # '!"' < '#$' < 'zy'


@functools.lru_cache(maxsize=None)
def ties_at_the_top():
    """Three pairs of count L - 1 each.  The lexically largest, `zy`, stands at position 0; `#$` first occurs at position
    1,024, the first of the second span; `!"`, the lexically smallest, comes last."""
    f = [_fill(20 + i, n, 23, 97, 9) for i, n in enumerate((1022, 300, 200, 150, 150, 280))]
    chunks = [b"zy"] + f[0] + [b"#$"] + f[1] + [b'!"'] + f[2] + [b'c!"', b"e#$"] + f[3] + [b"zyf"] + f[4] + [b'!"d'] + f[5]
    heavy = {b"zy": 1 << 30, b"#$": 1 << 30, b'!"': 1 << 30, b'c!"': (1 << 29) - 1, b'!"d': 1 << 29,
             b"e#$": (1 << 30) - 1, b"zyf": (1 << 30) - 1}
    weights = [heavy.get(c, 1) for c in chunks]
    return _case(chunks, weights, 256 + 8)


def prior_then_limits():
    """sum_beyond_2_32("b"), to be continued from its own first N_PRIOR merges (prior_merges): the pair count then
    reads a stream that holds ids of 256 and above."""
    return sum_beyond_2_32("b")


# name -> builder, the cases that train (the ladder's first two counts in every layout) and all of them
TRAINS = collections.OrderedDict()
TRAINS["sum_beyond_2_32-a"] = functools.partial(sum_beyond_2_32, "a")
TRAINS["sum_beyond_2_32-b"] = functools.partial(sum_beyond_2_32, "b")
TRAINS["many_distinct_pairs"] = many_distinct_pairs
TRAINS["ties_at_the_top"] = ties_at_the_top
for _layout in LAYOUTS:
    for _c, _name in ((L - 2, "L-2"), (L - 1, "L-1")):
        TRAINS["ladder-%s-%s" % (_layout, _name)] = functools.partial(ladder, _c, _layout)

OVERFLOWS = [(c, layout) for layout in LAYOUTS for c in LADDER_COUNTS if c >= L]


@functools.lru_cache(maxsize=None)
def trained(name, first_mode):
    """The reference of TRAINS[name], computed once."""
    chunks, weights, vocab, expect = TRAINS[name]()
    assert expect == "trains"
    return reference(chunks, weights, vocab, first_mode)


@functools.lru_cache(maxsize=None)
def trained_from_prior(first_mode):
    """(prior merges, Reference of the continuation) of prior_then_limits."""
    chunks, weights, vocab, _ = prior_then_limits()
    prior = trained("sum_beyond_2_32-b", first_mode).merges[:N_PRIOR]
    return prior, reference(chunks, weights, vocab, first_mode, prior=prior)


def stream_of(seqs):
    """Token sequences -> (tokens uint32, ends uint8) as Trainer.stream() gives them."""
    toks = np.array([t for s in seqs for t in s], dtype=np.uint32)
    ends = np.zeros(len(toks), dtype=np.uint8)
    ends[np.cumsum([len(s) for s in seqs]) - 1] = 1
    return toks, ends
