"""Case generators for the span-parallel encode (csrc/encode.hip) and, through the same shapes, the 32-bit merge loop
(csrc/wide.hip).  No GPU, no pytest: plain functions that return lists of Case(data, chunk_off, merges, name, ...).

Both loops cut the token array into spans of SPAN tokens and link them with single-workgroup scans of SLICES threads;
thread t of a scan owns per = ceil(n_spans / SLICES) consecutive spans (its slice).  The cases are laid out around
those two numbers: spans whose every position is a candidate (they hand the incoming run parity on), slices made of
such spans only, chunk ends next to slice edges, NUL-led chunks across lane-group, span and slice edges, and lookup
tables whose probe chains wrap the table end.

Every generator takes `scale` (1 = the kernels' real geometry; 1/32 divides span length and slice count by 32, which
keeps the structure -- the same per values, the same positions relative to span and slice edges -- at a size a
brute-force encode in Python can judge: tests/test_encode_cases_cpu.py)."""
from collections import namedtuple

import numpy as np

import oracle as O

SPAN = 1024            # tokens one wave walks: kSpan (csrc/span.h)
SLICES = 1024          # threads of a scan = slices the spans are dealt into: kScanThreads
GROUP = 64             # lanes of a wave: the unit of the ballots inside a span

# name: for messages.  tok: None, or (text, special_tokens_file) that reaches the same chunks through a Tokenizer
# with the basic encoder (pattern ""): the parts between special tokens are the chunks, a special token travels as
# the chunk "\0<id>".
Case = namedtuple("Case", "data chunk_off merges name tok", defaults=(None,))


def geometry(scale=1.0):
    """(span, slices, group) at this scale."""
    return max(int(SPAN * scale), 8), max(int(SLICES * scale), 4), max(int(GROUP * scale), 2)


def _u8(b):
    return np.frombuffer(bytes(b), dtype=np.uint8) if not isinstance(b, np.ndarray) else b


def _off(cuts, n):
    cuts = sorted(set(int(c) for c in cuts if 0 < c < n))
    return np.array([0] + cuts + [n], dtype=np.uint64)


# ---- runs ---------------------------------------------------------------------------------------------------------

N_SPANS = ((1, -1), (1, 0), (1, 1), (2, -1), (2, 0), (2, 1), (3, 1), (5, 1))     # n_spans = a * SLICES + b
DOUBLINGS = 22


def run_merges():
    """(a,a) -> 256, (256,256) -> 257, ... 22 deep, then (a,b) -> 278, (b,a) -> 279: in `abab..` and `aabaab..` every
    position is a candidate and the replaced ones alternate."""
    m = [(97, 97)] + [(256 + k, 256 + k) for k in range(DOUBLINGS - 1)] + [(97, 98), (98, 97)]
    return np.array(m, dtype=np.uint32)


def slice_edge_cuts(n, span, slices, rot):
    """Chunk ends at k * span * per + {-1, 0, +1} bytes for the first, a middle and the last slice in use; `rot`
    turns which of the three offsets goes with which slice, so that three values of rot give all nine."""
    n_spans = -(-n // span)
    per = -(-n_spans // slices)
    used = -(-n_spans // per)
    ks = sorted(set(k for k in (1, used // 2, used - 1) if k >= 1))
    return [k * span * per + (-1, 0, 1)[(j + rot) % 3] for j, k in enumerate(ks)]


def run_cases(scale=1.0):
    span, slices, _ = geometry(scale)
    merges = run_merges()
    out = []
    for si, (a, b) in enumerate(N_SPANS):
        n_spans = a * slices + b
        for ki, period in enumerate((b"a", b"ab", b"aab")):
            for variant in range(4):                      # 0: one chunk; 1..3: chunk ends at the slice edges
                # 0, 1 or 2 bytes that are no candidates first: the run starts at an even or an odd position, and
                # (with one or two) the first span is not full while every span behind it is
                lead = (si + ki + variant) % 3
                # the last span holds 1, span / 2 + 1 or span tokens
                n = (n_spans - 1) * span + (1, span // 2 + 1, span)[(si + variant) % 3]
                body = np.tile(_u8(period), (n - lead) // len(period) + 1)[:n - lead]
                data = np.concatenate([np.full(lead, 122, dtype=np.uint8), body])
                off = None if variant == 0 else _off(slice_edge_cuts(n, span, slices, variant - 1), n)
                name = "run:%s n_spans=%d per=%d lead=%d n=%d %s" % (
                    period.decode(), n_spans, -(-n_spans // slices), lead, n,
                    "one chunk" if off is None else "cuts=%s" % off[1:-1].tolist())
                assert -(-n // span) == n_spans
                out.append(Case(data, off, merges, name))
    return out


# ---- fuzz ---------------------------------------------------------------------------------------------------------

MAX_CHUNKS = 100000      # (the oracle encodes chunk by chunk in a Python loop)


def fuzz_case(rng, scale=1.0):
    """As test_encode_fuzz_against_oracle: small alphabet, merges trained by the oracle on other data of the same
    kind (every depth of merge occurs), optionally runs, optionally random chunks; 1-6 Mi bytes at scale 1."""
    alpha = int(rng.integers(2, 20))
    train = rng.integers(97, 97 + alpha, size=int(rng.integers(500, 20000)), dtype=np.uint8)
    merges, _ = O.train(train, 256 + int(rng.integers(5, 300)))
    n = max(int(int(rng.integers(1 << 20, (6 << 20) + 1)) * scale), 2)
    data = rng.integers(97, 97 + alpha, size=n, dtype=np.uint8)
    runs = bool(rng.integers(0, 2))
    if runs:
        data = np.repeat(data[:n // 8 + 1], rng.integers(1, 16, size=n // 8 + 1))[:n]
    data = np.ascontiguousarray(data)
    n = len(data)
    off = None
    if rng.integers(0, 2):
        mean = int(rng.integers(2, 50))
        cuts = np.unique(rng.integers(1, max(n, 2), size=min(max(n // mean, 1), MAX_CHUNKS - 1)))
        off = np.concatenate([[0], cuts[cuts < n], [n]]).astype(np.uint64)
    name = "fuzz: n=%d alphabet=%d merges=%d runs=%d chunks=%d" % (n, alpha, len(merges), runs,
                                                                  1 if off is None else len(off) - 1)
    return Case(data, off, merges, name)


def deep_block(seed, n):
    """One block of the fuzz kind with deep merges (alphabet 3, runs, 300 merges): the tile of the > 4 GiB case."""
    rng = np.random.default_rng(seed)
    train = np.repeat(rng.integers(97, 100, size=4000, dtype=np.uint8), rng.integers(1, 8, size=4000))
    merges, _ = O.train(np.ascontiguousarray(train), 256 + 300)
    data = np.repeat(rng.integers(97, 100, size=n, dtype=np.uint8), rng.integers(1, 8, size=n))[:n]
    return np.ascontiguousarray(data), merges


# ---- NUL-led chunks -----------------------------------------------------------------------------------------------

INT_MAX = 2147483647
MAX_DEVICE_ID = 0x7FFFFFFD                 # ids from 0x7FFFFFFE on are MBPE_ERR_ARG on the device (mbpe.h)
SPECIAL_IDS = (0, 7, 12, 49, 300, 65535, 70000, 100257, 1000000007, MAX_DEVICE_ID)
BLANKS = b" \t\n\v\f\r"


def special_name(i):
    return b"<|s%d|>" % i


def special_file():
    return b"".join(special_name(i) + b" %d\n" % i for i in SPECIAL_IDS)


def nul_merges():
    """Pairs over the bytes a marker is written with (NUL, digits, blanks, sign), over ordinary text, and (id, byte),
    (byte, id), (id, id) for the ids the markers stand for: a marker whose bytes were merged, or whose id merged with
    a neighbour across the chunk end, shows in the output."""
    m = [(49, 50), (50, 51), (48, 48), (57, 57), (32, 49), (0, 49), (0, 50), (0, 32), (0, 43), (43, 55), (0, 97), (0, 48),
         (97, 98), (98, 99), (99, 97), (49, 97), (99, 49), (32, 32), (48, 49), (55, 48), (52, 55), (50, 49), (52, 50)]
    m += [(256, 51), (268, 99), (256 + len(m) + 1, 256 + len(m) + 1), (258, 258)]     # (12)(3), (ab)(c), (abc)(abc), (00)(00)
    for i in SPECIAL_IDS:
        m += [(i, 97), (99, i), (i, i), (i, 0), (51, i)]
    return np.array(m, dtype=np.uint32)


def marker_remainders(rng):
    """What may follow the NUL: (remainder, comment).  Each parses, or fails to, as std::stoi has it."""
    big = int(rng.integers(1 << 20, MAX_DEVICE_ID))
    return [
        (b"0", "id 0"), (b"12", "two digits"), (b"300", "id above the bytes"), (b"%d" % big, "a large id"),
        (b"%d" % MAX_DEVICE_ID, "the largest id the device takes"), (b"0000000012", "leading zeros"),
        (b" 12", "a leading blank"), (BLANKS + b"7", "every blank stoi skips"), (b"+7", "a plus sign"),
        (b" \t+300", "blanks and a sign"), (b"-0", "minus zero"),
        (b"12abc", "digits, then garbage"), (b"12 12", "digits, a blank, digits"), (b"7\x0012", "digits, NUL, digits"),
        (b"70000.5", "digits, a point"),
        (b"abc", "garbage only: stays bytes"), (b"", "nothing: the NUL byte alone"), (b"+", "a sign alone"),
        (b" ", "a blank alone"), (b"+-7", "two signs"), (b"\x0012", "a second NUL first"), (b"a12", "a letter first"),
        (b"%d" % (INT_MAX + 1), "INT_MAX + 1: out of range, stays bytes"), (b"%d" % (INT_MAX + 3), "INT_MAX + 3"),
        (b"4294967296", "2^32"), (b"4294967297", "2^32 + 1"), (b"4294967308", "2^32 + 12"),
        (b"9" * 20, "twenty nines"), (b"0" * 20 + b"12", "twenty zeros, then 12"),
    ]


def _pad_marker(rem, length, rng):
    """The chunk NUL + rem stretched to at least `length` bytes without changing what it parses to: blanks in front
    (stoi skips them, and they rescue no remainder that fails), or a letter and anything behind it."""
    need = length - 1 - len(rem)
    if need <= 0:
        return b"\0" + rem
    if rng.integers(0, 2):
        return b"\0" + bytes(rng.choice(list(BLANKS), size=need).astype(np.uint8)) + rem
    return b"\0" + rem + b"x" + bytes(rng.choice(list(b"abc 12\x00z"), size=need - 1).astype(np.uint8))


def _plain(rng, n):
    """An ordinary chunk of n bytes: letters and digits the merges know (it never starts with NUL)."""
    return bytes(rng.choice(list(b"abcabcabc123 0479"), size=n).astype(np.uint8))


class _Text:
    """Pieces of a text: ordinary chunks, NUL-led chunks with any remainder, special tokens (NUL + decimal id)."""

    def __init__(self, rng):
        self.rng, self.pieces, self.kinds, self.n = rng, [], [], 0

    def add(self, b, kind):
        if len(b):
            self.pieces.append(bytes(b))
            self.kinds.append(kind)
            self.n += len(b)

    def plain(self, n):
        self.add(_plain(self.rng, n), "p")

    def special(self, i=None):
        i = SPECIAL_IDS[int(self.rng.integers(0, len(SPECIAL_IDS)))] if i is None else i
        self.add(b"\0%d" % i, "s")

    def fill_to(self, pos, reachable):
        """Ordinary chunks up to byte offset `pos` (in one piece when the text must be reachable through a Tokenizer:
        two ordinary parts side by side would be one chunk there)."""
        while self.n < pos:
            left = pos - self.n
            if left > 8192 and not reachable:
                self.plain(left - 4096)                             # (a long way: one long chunk, then short ones)
            else:
                self.plain(left if reachable or left < 4 else min(left, int(self.rng.integers(1, 40))))

    def case(self, name, reachable):
        data = _u8(b"".join(self.pieces))
        off = np.concatenate([[0], np.cumsum([len(p) for p in self.pieces])]).astype(np.uint64)
        tok = None
        if reachable:
            by_id = {b"\0%d" % i: special_name(i) for i in SPECIAL_IDS}
            for k in range(1, len(self.kinds)):
                assert "s" in (self.kinds[k - 1], self.kinds[k]), "two parts side by side are one chunk for a Tokenizer"
            text = b"".join(by_id[p] if k == "s" else p for p, k in zip(self.pieces, self.kinds))
            assert all(b"<|" not in p for p, k in zip(self.pieces, self.kinds) if k != "s")
            tok = (text, special_file())
        return Case(data, off, nul_merges(), "nul: " + name, tok)


def _straddle_text(rng, edges, total, reachable, lengths):
    """Markers laid across every offset of `edges` (a marker of length L starts 1 .. L-1 bytes before the edge), the
    first and the last chunk markers too, pairs and triples of markers in between."""
    t = _Text(rng)
    rems = marker_remainders(rng)
    ri = int(rng.integers(0, len(rems)))
    t.special()                                                   # first chunk
    t.special()                                                   # two in a row
    for ei, edge in enumerate(sorted(edges)):
        length = lengths[ei % len(lengths)]
        rem = rems[ri % len(rems)][0]
        ri += 1
        m = _pad_marker(rem, length, rng)
        before = int(rng.integers(1, len(m))) if len(m) > 1 else 0
        start = edge - before
        if start <= t.n + 2:
            continue                                              # (edges closer than the markers are long)
        if reachable:
            t.fill_to(start - len(b"\0%d" % SPECIAL_IDS[ei % len(SPECIAL_IDS)]), True)
            t.special(SPECIAL_IDS[ei % len(SPECIAL_IDS)])         # the quirk chunk is the part right behind a special
            if t.n != start:
                continue
        else:
            t.fill_to(start, False)
        t.add(m, "q")
        assert start < edge <= t.n or len(m) == 1
        if ei % 3 == 0:
            t.special()
            t.special()
            t.special()                                           # three in a row
        elif ei % 3 == 1 or reachable:
            t.special()
    if t.kinds[-1] != "s" and reachable:
        t.special()
    t.fill_to(max(total, t.n + 1), reachable)
    t.special()                                                   # last chunk
    return t


def nul_cases(rng, scale=1.0):
    span, slices, group = geometry(scale)
    out = []
    # markers across the lane-group edges of the first spans and across span edges
    edges = [group * k for k in range(1, 2 * span // group + 1)] + [span * k for k in (3, 4, 5)]
    for reachable in (False, True):
        for lengths in ((2, 3, 5, 12), (group + 1, group + 9, 200 if scale == 1.0 else 3 * group), (1, 2, 200, 31)):
            t = _straddle_text(rng, edges, 6 * span + 3, reachable, lengths)
            out.append(t.case("group and span edges, marker lengths %s%s" % (lengths, ", via Tokenizer" * reachable),
                              reachable))
    # more than SLICES spans: markers across the slice edges (per = 2) and the span edges next to them
    n_spans = slices + slices // 2 + 1
    per = 2
    ks = (1, 2, slices // 4, slices // 2, (n_spans - 1) // per)
    edges = sorted(set(k * per * span + d * span for k in ks for d in (-1, 0, 1) if k * per + d > 0))
    for reachable in (False, True):
        t = _straddle_text(rng, edges, (n_spans - 1) * span + span // 3, reachable,
                           (2, 7, group + 3, 200 if scale == 1.0 else 3 * group, 12))
        c = t.case("slice edges, n_spans=%d per=%d%s" % (-(-t.n // span), per, ", via Tokenizer" * reachable), reachable)
        assert -(-len(c.data) // (span * slices)) == per
        out.append(c)
    # a random mixture: a third of the chunks NUL-led, every kind of remainder, lengths 1 .. 200
    t = _Text(rng)
    rems = marker_remainders(rng)
    while t.n < max(40 * span, 20000):
        r = int(rng.integers(0, 6))
        if r < 2:
            rem = rems[int(rng.integers(0, len(rems)))][0]
            length = int(rng.integers(1, 201)) if rng.integers(0, 4) == 0 else 0
            t.add(_pad_marker(rem, length, rng), "q")
        elif r == 2:
            t.special()
        else:
            t.plain(int(rng.integers(1, 60)))
    out.append(t.case("random mixture, %d chunks" % len(t.pieces), False))
    return out


def nul_error_cases():
    """NUL-led chunks whose id the device refuses (MBPE_ERR_ARG: ids from 0x7FFFFFFE on, negative values) and the host
    takes as a token: (data, chunk_off, merges, name)."""
    out = []
    for rem in (b"2147483646", b"2147483647", b"-1", b"-12", b"-2147483648", b" \t-7abc", b"+2147483647"):
        for before, after in ((b"", b""), (b"abc", b"abc"), (b"abc" * 700, b"")):
            pieces = [p for p in (before, b"\0" + rem, after) if p]
            data = _u8(b"".join(pieces))
            off = np.concatenate([[0], np.cumsum([len(p) for p in pieces])]).astype(np.uint64)
            out.append(Case(data, off, nul_merges(), "nul error: %r after %d bytes" % (rem, len(before))))
    return out


# ---- lookup tables ------------------------------------------------------------------------------------------------

M64 = (1 << 64) - 1
MAX_SIDE = (1 << 31) - 3                  # "Token ids must stay below 2^31 - 2" (mbpe.h)


def enc_hash(key, shift):
    # csrc/span.h, pair_hash:  (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> shift)
    return ((key * 0x9E3779B97F4A7C15) & M64) >> shift


def table_bits(n_merges):
    # encode.hip, encode_chunks:  bits = 4; while ((1ull << bits) < 2ull * n_merges + 2) ++bits;
    bits = 4
    while (1 << bits) < 2 * n_merges + 2:
        bits += 1
    return bits


def build_table(merges):
    """The open-addressing table encode_chunks builds on the host -> (slots: key or None, bits)."""
    bits = table_bits(len(merges))
    cap = 1 << bits
    slots = [None] * cap
    for a, b in merges:
        key = (int(a) << 32) | int(b)
        h = enc_hash(key, 64 - bits)
        while slots[h] is not None and slots[h] != key:
            h = (h + 1) & (cap - 1)
        slots[h] = key
    return slots, bits


def wrapped_keys(slots, bits):
    """Keys whose home slot is one of the last two and that are stored before it: their chain wrapped the table end."""
    cap = 1 << bits
    out = []
    for at, key in enumerate(slots):
        if key is not None:
            home = enc_hash(key, 64 - bits)
            if home >= cap - 2 and at < home:
                out.append(key)
    return out


def tail_chain(slots, bits):
    """Keys with a home in the last two slots, and the slots the chain that starts at cap - 2 occupies."""
    cap = 1 << bits
    homes = [k for k in slots if k is not None and enc_hash(k, 64 - bits) >= cap - 2]
    length = 0
    while length < cap and slots[(cap - 2 + length) & (cap - 1)] is not None:
        length += 1
    return homes, length


FIRST_A = tuple(range(0x40, 0x80))         # first bytes of the first layer's pairs
FIRST_B = tuple(range(0x80, 0xC0))         # second bytes: (second, first) is never a pair, so pass 1 is exactly layer 1


def _layers(rng, n1, n2, n3, n_fill):
    """Merges in the order: layer 1 (byte pairs -> ids 256 ..), fillers (sides no text produces: they only occupy slots
    and lengthen chains), layer 2 (pairs of layer-1 ids), layer 3 (pairs of layer-2 ids).  -> merges, ids of the layers"""
    side = int(np.ceil(np.sqrt(n1)))
    l1 = [(FIRST_A[k // side], FIRST_B[k % side]) for k in range(n1)]
    id1 = list(range(256, 256 + n1))
    total = n1 + n_fill + n2 + n3
    fill = set()
    while len(fill) < n_fill:
        a, b = (int(v) for v in rng.integers(256 + total, MAX_SIDE + 1, size=2))
        fill.add((a, b) if len(fill) % 3 else (a, MAX_SIDE))
    fill = sorted(fill)
    l2 = set()
    while len(l2) < n2:
        l2.add((id1[int(rng.integers(0, n1))], id1[int(rng.integers(0, n1))]))
    l2 = sorted(l2)
    rng.shuffle(l2)
    l2 = [tuple(int(v) for v in p) for p in l2]
    id2 = list(range(256 + n1 + n_fill, 256 + n1 + n_fill + n2))
    l3 = set()
    lo = max(n2 // 2, n2 - 4096)
    while len(l3) < n3 and n2:
        # (the top of layer 2: the sides of layer 3 are the highest ids a text can make)
        l3.add((id2[int(rng.integers(lo, n2))], id2[int(rng.integers(lo, n2))]))
    l3 = sorted(l3)
    merges = np.array(l1 + fill + l2 + l3, dtype=np.uint32).reshape(-1, 2)
    return merges, l1, l2, l3


def _expand(ids, merges):
    """ids -> bytes through the merges (256 + k -> merges[k])."""
    out = []
    stack = list(reversed(ids))
    while stack:
        t = stack.pop()
        if t < 256:
            out.append(t)
        else:
            a, b = merges[t - 256]
            stack.append(int(b))
            stack.append(int(a))
    return np.array(out, dtype=np.uint8)


def _lookup_case(rng, n, n_ids, name, want_wrap=False):
    if n == 1:
        n1, n_fill, n2, n3 = 1, 0, 0, 0
    elif n <= 8:
        n1, n_fill, n2, n3 = 3, 1, n - 5, 1
    elif n <= 64:
        n1, n_fill, n2, n3 = 36, 0, n - 36 - 4, 4
    else:
        n1 = 4096
        n_fill = n // 20
        n3 = (n - n1 - n_fill) // 3
        n2 = n - n1 - n_fill - n3
    extra = []
    if want_wrap:
        # choose layer 2 so that six of its pairs hash to the last two slots of the table (the capacity follows from n
        # alone); absent pairs that hash there too go into the text
        bits = table_bits(n)
        cap = 1 << bits
        id1 = list(range(256, 256 + n1))
        home = [(x, y) for x in id1 for y in id1 if enc_hash((x << 32) | y, 64 - bits) >= cap - 2]
        assert len(home) >= 12, "not enough pairs of layer-1 ids with a home in the last two slots"
        chain, extra = home[:6], home[6:]
        merges, l1, l2, l3 = _layers(rng, n1, n2 - len(chain), 0, n_fill)
        l2 = chain + [p for p in l2 if p not in set(home)]
        ids2 = range(256 + n1 + n_fill, 256 + n1 + n_fill + len(l2))
        l3 = [(ids2[0], ids2[1]), (ids2[2], ids2[3]), (ids2[4], ids2[5]), (ids2[1], ids2[0])][:n - n1 - n_fill - len(l2)]
        merges = np.array(l1 + [tuple(p) for p in merges[n1:n1 + n_fill].tolist()] + l2 + l3, dtype=np.uint32).reshape(-1, 2)
        assert len(merges) == n
    else:
        merges, l1, l2, l3 = _layers(rng, n1, n2, n3, n_fill)
    assert len(merges) == n, (len(merges), n)
    id1 = list(range(256, 256 + n1))
    base2 = 256 + n1 + n_fill
    base3 = base2 + len(l2)
    ids = []
    while len(ids) < n_ids:
        r = int(rng.integers(0, 8))
        if r < 3 and l2:
            ids += l2[int(rng.integers(0, len(l2)))]                          # a present pair of layer 2
        elif r < 5 and l3:
            k = int(rng.integers(0, len(l3)))
            ids += [base3 + k] if rng.integers(0, 2) else list(l3[k])         # a present pair of layer 3 (or its id)
        elif r == 5 and extra:
            ids += extra[int(rng.integers(0, len(extra)))]                    # an absent pair that probes the chain
        else:
            ids += [id1[int(rng.integers(0, n1))] for _ in range(int(rng.integers(1, 4)))]
    if n3 and not want_wrap:
        ids += [base3 + len(l3) - 1] * 3                                      # the last merge of the table occurs
    data = _expand(ids, merges.tolist())
    return Case(np.ascontiguousarray(data), None, merges, "lookup: %s, %d merges, %d bytes" % (name, n, len(data)))


def lookup_cases(scale=1.0):
    """Synthetic merges tables (encode only looks pairs up): a first layer of byte pairs makes the ids 256 .., the
    layers above are pairs of those ids, so the lookups with high sides happen from pass 2 on."""
    rng = np.random.default_rng(77)
    n_ids = max(int((1 << 18) * scale), 64)
    out = [_lookup_case(rng, n, n_ids, "size %d" % n) for n in (1, 7, 8, (1 << 15) - 1, 1 << 15, 100000)]
    out.append(_lookup_case(rng, 50, n_ids, "chain wraps the table end", want_wrap=True))
    return out


def all_cases(scale=1.0):
    """Every case of this file (the error cases apart), in a fixed order."""
    out = run_cases(scale)
    out += [fuzz_case(np.random.default_rng(4200 + s), scale) for s in range(4)]
    out += nul_cases(np.random.default_rng(4300), scale)
    out += lookup_cases(scale)
    return out
