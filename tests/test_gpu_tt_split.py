"""The split route of fused passes whose byte batch has (t,t) members (option "tt_split"; k_tt_split_plan in kernels.hip):
the pass runs without the (t,t) code and defers the tiles in or next to a run of a member's token to a list pass.

Every case runs the same training three ways -- "tt_split" 0 (the whole-stream (t,t) instantiation), 1 (split wherever the
route exists) and -1 (the default rule) -- one sequence at a time, and compares merges, counts, live tokens and the whole
pair table after every sequence with an oracle state advanced by as many merges; the final token streams of the three runs
must be equal.  With 1 the case asserts that split passes ran and deferred tiles, so it cannot pass on the old route.

How the corpora are made.  The route is never the frequent-pair instantiation's (top count x 8192 >= live tokens), a batch
only takes candidates of nearly equal counts, and its members must not share a token.  So a corpus here is a background
in which every pair is rare -- walks x, x + d, x + 2d, ... over 197 filler bytes, one per stride d, repeated `reps` times:
every background pair occurs `reps` times -- with the features of special bytes (198 and up) written over it, and every
pair meant for the batch is then brought to one count (`level`) by isolated occurrences in tiles of their own, few enough
that the top count stays below live tokens / 8192.  A decoy pair (198, 199), one occurrence more than the others and far
from every feature, is the first merge whether or not it is taken alone, so the first split pass still sees the bytes
as they were loaded wherever it matters: before the first merge a slot is a byte, byte i sits at slot i % 512 of tile
i // 512, and the host can say which tiles must defer (`_deferred`).

Three of the cases the split was specified with cannot take the route at the sizes named, because of the frequent-pair
rule: a corpus that is all one byte, a run of 1,100 equal bytes in less than 9 M tokens, and random bytes over three
symbols at 8 - 64 Ki bytes.  Their substitutes here: two stretches of 1,100 equal bytes in a 9.1 M background (every
tile they cover defers: the long list), and random strings over three special bytes as islands in the background.
An empty tile is never deferred: neither kernel calls the tile function for a tile without live tokens."""
import numpy as np
import pytest

import mbpe
import oracle as O

pytestmark = pytest.mark.gpu

OPTS = {"tt_split": -1, "fused_min": 24, "chunk_barrier": -1}           # the defaults, put back after every run
P = 197          # filler bytes 0 .. 196; 198 .. 255 are the special ones
TILE = 512
DECOY = (198, 199)


@pytest.fixture(scope="module")
def tr():
    t = mbpe.Trainer(0)
    yield t
    t.close()


def _background(reps):
    x = np.arange(P)
    one = np.concatenate([(x * d + d) % P for d in range(1, P)]).astype(np.uint8)
    return np.tile(one, reps)


class _Corpus:
    def __init__(self, reps=10):
        self.data = _background(reps)
        self.cuts = []                      # chunk ends (byte offsets)

    def put(self, tile, slot, values):
        at = tile * TILE + slot
        assert at + len(values) + 2 * TILE < len(self.data)
        self.data[at:at + len(values)] = values
        return at

    def count(self, a, b):
        hit = (self.data[:-1] == a) & (self.data[1:] == b)
        for c in self.cuts:
            hit[c - 1] = False              # (no pair across a chunk end)
        return int(hit.sum())

    def level(self, pairs, target, tile):
        """Brings every pair to `target` occurrences: isolated ones, 50 to a tile, from `tile` on; tiles are left free
        behind each pair's.  -> the next free tile."""
        for a, b in pairs:
            need = target - self.count(a, b)
            assert need >= 0, (a, b, need)
            for e in range(need):
                self.put(tile + e // 50, 100 + 7 * (e % 50), [a, b])
            assert self.count(a, b) == target, (a, b)
            tile += (need + 49) // 50 + 2
        return tile

    def fill(self, values, n, tile):
        """n isolated copies of `values`, 50 to a tile, from `tile` on.  -> the next free tile."""
        for e in range(n):
            self.put(tile + e // 50, 100 + 9 * (e % 50), values)
        return tile + (n + 49) // 50 + 2

    def finish(self, pairs, target, tile):
        tile = self.level(pairs, target, tile + 4)
        tile = self.level([DECOY], target + 1, tile + 4)
        assert (target + 1) * 8192 < len(self.data), "the top pair would be a frequent one"
        return tile

    def off(self):
        if not self.cuts:
            return None
        return np.array([0] + sorted(self.cuts) + [len(self.data)], dtype=np.uint64)


def _deferred(data, members):
    """The tiles a split pass over the loaded bytes must defer: tile T looks up the pairs that start at its slots, the
    two before them -- (p2, p1), (p1, first) -- and (n1, n2) behind (last, n1): bytes 512 T - 2 .. 512 T + 512."""
    tiles = set()
    n_tiles = (len(data) + TILE - 1) // TILE
    for i in np.flatnonzero((data[:-1] == data[1:]) & np.isin(data[:-1], list(members))):
        i = int(i)
        for t in range(max(0, -(-(i - TILE) // TILE)), min(n_tiles - 1, (i + 2) // TILE) + 1):
            tiles.add(t)
    return tiles


def _keys(a, b):
    return (a.astype(np.uint64) << np.uint64(32)) | b.astype(np.uint64)


def _table(tr, ost, where):
    a, b, c = tr.pairs()
    oa, ob, oc = ost.table()
    live = oc != 0
    ok, oc = _keys(oa[live], ob[live]), oc[live]
    order = np.argsort(ok)
    ok, oc = ok[order], oc[order]
    keep = c != 0
    dk, dc = _keys(a[keep], b[keep]), c[keep]
    order = np.argsort(dk)
    dk, dc = dk[order], dc[order]
    assert np.array_equal(dk, ok), "pairs with a count differ " + where
    assert np.array_equal(dc, oc), "counts differ " + where


def _run(tr, data, off, vocab, mode, **opts):
    for k, v in dict(OPTS, fused_min=2, tt_split=mode, **opts).items():
        tr.set_option(k, v)
    ost = O.State(data, off)
    try:
        tr.load_corpus(data, off)
        tr.train_begin(vocab)
        k, seqs = 0, []
        while True:
            d = tr.train_sequences(1)
            if d == 0:
                break
            tops = []
            for j in range(d):
                top = ost.top()
                assert top is not None
                tops.append(top)
                ost.merge(top[0], top[1], 256 + k + j)
            m, c = tr.train_result()
            where = "tt_split %d after merge %d (+%d)" % (mode, k, d)
            assert [(int(m[k + j][0]), int(m[k + j][1]), int(c[k + j])) for j in range(d)] == tops, where
            st = tr.stats()
            assert st["n_live"] == len(ost.stream()[0]), where
            _table(tr, ost, where)
            seqs.append((k, d, st["n_tt_split"], st["tt_deferred_tiles"], st["n_fused_dropped"]))
            k += d
        assert k == vocab - 256
        toks, ends = tr.stream()
        assert np.array_equal(toks, np.asarray(ost.stream()[0])), "final stream, tt_split %d" % mode
        m, c = tr.train_result()
        return seqs, m, c, toks, tr.stats()
    finally:
        ost.close()
        for k, v in OPTS.items():
            tr.set_option(k, v)


def _three_ways(tr, corpus, vocab, count=True, **opts):
    """-> the three runs by mode.  count: the first split pass of the forced run comes behind the decoy's merge at the
    most, and the tiles it defers are the ones the host finds for the (t,t) pairs merged in that sequence."""
    data, off = corpus.data, corpus.off()
    res = {mode: _run(tr, data, off, vocab, mode, **opts) for mode in (0, 1, -1)}
    for mode in (1, -1):
        assert np.array_equal(res[0][1], res[mode][1]) and np.array_equal(res[0][2], res[mode][2]), mode
        assert np.array_equal(res[0][3], res[mode][3]), mode
    assert res[0][4]["n_tt_split"] == 0 and res[0][4]["tt_deferred_tiles"] == 0
    seqs, m = res[1][0], res[1][1]
    st = res[1][4]
    assert st["n_tt_split"] > 0 and st["tt_deferred_tiles"] > 0, (seqs, st)
    if count:
        splits, tiles = 0, 0
        for k, d, n_split, n_tiles, _ in seqs:
            if n_split > splits:
                break
            splits, tiles = n_split, n_tiles
        assert n_split == splits + 1, seqs
        assert [(int(a), int(b)) for a, b in m[:k]] in ([], [DECOY]), (seqs, m[:k])
        members = [int(a) for a, b in m[k:k + d] if a == b]
        assert members and max(members) < 256, (seqs, m[k:k + d])
        assert n_tiles - tiles == len(_deferred(data, members)), (seqs, members)
    return res


def test_runs_at_tile_edges(tr):
    """Runs of 2 .. 9 equal bytes, one special byte per length, each length starting at slots 509 .. 513 of a tile: before,
    across and after the edge, in both parities.  Eight (t,t) members, 40 pairs each, over a background of 10."""
    c = _Corpus()
    tile = 3
    for length in range(2, 10):
        for slot in range(509, 514):
            c.put(tile, slot, [200 + length] * length)
            tile += 5
    c.finish([(200 + length, 200 + length) for length in range(2, 10)], 40, tile)
    res = _three_ways(tr, c, 256 + 13)
    assert len([1 for a, b in res[1][1] if a == b]) >= 8


def test_run_across_an_edge(tr):
    """One run of two across a tile edge (slots 511 and 0): exactly that tile and the next one defer for it, their
    neighbours do not; every other occurrence lies inside a tile and defers that tile alone."""
    c = _Corpus()
    c.put(10, 511, [201, 201])
    assert _deferred(c.data, [201]) == {10, 11}
    c.finish([(201, 201), (202, 202), (204, 205)], 40, 14)
    _three_ways(tr, c, 256 + 6)


def test_runs_longer_than_a_tile(tr):
    """Two stretches of 1,100 equal bytes (the scaled stand-in for "all one byte"): every tile a stretch covers defers,
    and the one before it.  1,099 pairs each ask for 9.1 M bytes of background, or the pass is the frequent-pair one."""
    c = _Corpus(236)
    c.put(20, 300, [201] * 1100)
    c.put(40, 0, [202] * 1100)
    assert _deferred(c.data, [201, 202]) == {20, 21, 22, 39, 40, 41, 42}
    c.finish([(204, 205)], 1099, 50)
    _three_ways(tr, c, 256 + 5)


@pytest.mark.parametrize("n", [2, 3, 16])
def test_members_side_by_side(tr, n):
    """2, 3 and 16 (kTTMax) (t,t) members in one batch, runs of different members adjacent to each other -- aabb,
    aaabbb -- inside a tile and across an edge."""
    c = _Corpus()
    t = [200 + i for i in range(n)]
    tile = 3
    for i in range(n):
        a, b = t[i], t[(i + 1) % n]
        c.put(tile, 200, [a, a, b, b])
        c.put(tile + 2, 510, [a, a, b, b])
        c.put(tile + 5, 300, [a, a, a, b, b, b])
        c.put(tile + 7, 508 + i % 4, [a, a, a, b, b, b])
        tile += 10
    c.finish([(x, x) for x in t] + [(220, 221)], 40, tile)
    res = _three_ways(tr, c, 256 + n + 4)
    assert len([1 for a, b in res[1][1] if a == b]) >= n


def test_run_next_to_another_members_match(tr):
    """A member's run directly next to a match of another member of the batch, on the left, on the right, on both
    sides, and with the touching point on either side of and across a tile edge."""
    c = _Corpus(20)
    a, x, y, u, v = 201, 204, 205, 206, 207
    tile = 3
    for feature in ([x, y, a, a], [a, a, x, y], [x, y, a, a, u, v], [u, v, a, a, a, x, y], [x, y, a, a, a, a, u, v]):
        c.put(tile, 250, feature)
        for slot in range(506, 513):
            tile += 3
            c.put(tile, slot, feature)
        tile += 3
    c.finish([(a, a), (202, 202), (x, y), (u, v)], 70, tile)
    _three_ways(tr, c, 256 + 8, count=False)


@pytest.mark.parametrize("barrier", [0, 1])
def test_chunked(tr, barrier):
    """Chunks, with the end bit (0) and with barrier slots (1): a chunk end inside a run, just before it and just behind
    it, the runs starting at slots 505 .. 514, so that the end also falls in runs that cross a tile edge.  (Barrier slots
    shift the later bytes by one slot each: the sweep of start slots still covers the edge.)"""
    c = _Corpus(30)      # (25 runs of a member hold up to 125 pairs: the level lies above that)
    tile = 3
    for where in (3, 0, 6, 1, 5):
        for slot in range(505, 515):
            t = 201 + slot % 2
            at = c.put(tile, slot, [t] * 6)
            c.cuts.append(at + where)
            tile += 2
    c.cuts.append(c.put(tile, 100, [204, 205, 201, 201]) + 2)
    c.finish([(201, 201), (202, 202), (204, 205)], 135, tile + 2)
    _three_ways(tr, c, 256 + 6, count=False, chunk_barrier=barrier)


def test_holes_in_later_passes(tr):
    """Two levels of members: the second level's runs lie next to the first level's, so its split pass, sequences later,
    defers prefix-form tiles with trailing holes whose neighbours are merged tokens."""
    c = _Corpus(80)
    tile = 3
    for a, b in ((201, 211), (202, 212)):
        for feature in ([a] * 4 + [b] * 2, [b, b, a, a, a], [a, a, b, b, b, a, a], [b] * 5 + [a] * 6 + [b] * 3):
            for slot in (200, 505, 509, 511):
                c.put(tile, slot, feature)
                tile += 2
        c.put(tile, 0, [a] * 200 + [b] * 40)         # (a tile that loses 100 slots in front of the second level's run)
        tile += 3
    tile = c.level([(211, 211), (212, 212), (214, 215)], 120, tile + 4)
    c.finish([(201, 201), (202, 202), (204, 205)], 340, tile)
    res = _three_ways(tr, c, 256 + 12)
    assert res[1][4]["n_tt_split"] >= 2, res[1][0]


def test_nearly_every_tile_deferred(tr):
    """The long list: a run of two across every tile edge of the first 704 tiles, 16 members in turn (44 runs each, as
    many as the frequent-pair rule lets a member of this corpus have): 705 of the 755 tiles are listed."""
    c = _Corpus()
    for tile in range(704):
        c.put(tile, 511, [200 + tile % 16] * 2)
    members = list(range(200, 216))
    assert _deferred(c.data, members) == set(range(705))
    assert all(c.count(t, t) == 44 for t in members) and 46 * 8192 < len(c.data)
    c.level([DECOY], 45, 716)
    res = _three_ways(tr, c, 256 + 19)
    assert res[1][4]["tt_deferred_tiles"] >= 705


def test_abandoned_split_pass(tr):
    """A split pass that validation abandons.  The selection passes a dependent candidate over only once it has learnt
    that such candidates lose occurrences (until then it cuts the batch there), and never in a training's first
    sequence, which takes whatever is independent.  So (199, 200), as frequent as the decoy, ends the first sequence
    behind the decoy, and the level below teaches: (246, 247) occurs only in "246 247 248", and (247, 248), passed over
    behind it, loses everything.  At the last level the batch takes (t,t) members and (210, 211), passes (211, 212) over
    -- it stands alone, never behind "210 211" -- and takes (220, 221) and (222, 223) behind it, at the same count and
    later in the order.  Validation finds (211, 212) as frequent as before and keeps the members in front of it; the
    stream is rewritten from the buffer the split pass read, with the tile list, the restored (t,t) members and the list
    pass's match counts behind it."""
    c = _Corpus(80)
    tile = 3
    for t in (201, 202):
        for slot in (200, 509, 510, 511, 512):
            c.put(tile, slot, [t] * 5)
            tile += 3
    tile = c.level([(201, 201), (202, 202), (210, 211), (211, 212), (220, 221), (222, 223)], 120, tile + 2)
    tile = c.fill([246, 247, 248], 340, tile + 2)
    assert c.count(246, 247) == 340 and c.count(247, 248) == 340
    tile = c.finish([(240, 241)], 340, tile)
    c.level([(199, 200)], 341, tile + 2)
    res = _three_ways(tr, c, 256 + 12, count=False)
    seqs = res[1][0]
    grew = [(b[2] > a[2], b[4] > a[4]) for a, b in zip([(0, 0, 0, 0, 0)] + seqs, seqs)]
    assert (True, True) in grew, (seqs, res[1][1], res[1][4])


@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5])
def test_fuzz_islands(tr, seed):
    """Random strings over three special bytes (many runs, many ties), as islands of 2 .. 40 bytes in the background,
    every second one laid over a tile edge.  The three (t,t) pairs are levelled; the six mixed pairs stay as they fell."""
    rng = np.random.default_rng(seed)
    c = _Corpus()
    tile, total = 3, 0
    while total < 240:
        n = int(rng.integers(2, 41))
        slot = int(rng.integers(500 - n // 2, 512)) if rng.integers(2) else int(rng.integers(0, 400))
        c.put(tile, slot, rng.integers(200, 203, n).astype(np.uint8))
        total += n
        tile += int(rng.integers(2, 5))
    top = max(c.count(a, b) for a in (200, 201, 202) for b in (200, 201, 202))
    assert top <= 44, top
    c.finish([(200, 200), (201, 201), (202, 202)], top, tile)
    _three_ways(tr, c, 256 + 14, count=False)
