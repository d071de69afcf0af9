"""The run before a tile on the split route (option "tt_split"): a split pass skips the run scan (k_run_partial /
k_run_final return at once) and its list pass -- or, when validation abandons the pass, k_rewrite_marked -- walks the
tile summaries back from the tile instead (run_before_tile_wave in kernels.hip, run_before.h).  The summary of the tile
before is in a register: a partial trailing run there is the answer; a tile that is one whole run starts the walk.

The corpora and the three-way comparison against the oracle (tt_split 0, 1 and -1, after every sequence) are those of
tests/test_gpu_tt_split.py; every case asserts that split passes ran.  Cases here are about where a run ends and how far
back it reaches: runs ending at slots 511, 512 and 513; runs of 600 .. 1,701 equal bytes, whose list pass walks across
one, two and three full tiles; chunk ends in, before and behind such runs; 16 members; an abandoned split pass; a
training whose second list is far longer, and one whose second list is far shorter, than its first; and a
frequent-pair batch, which keeps the scan.  Some cases run with "lockstep" 0: the host then enqueues every
kernel of a sequence without knowing the batch, as it does on a large corpus."""
import numpy as np
import pytest

import mbpe
import oracle as O
import test_gpu_tt_split as S

pytestmark = pytest.mark.gpu

TILE = S.TILE


@pytest.fixture(scope="module")
def tr():
    t = mbpe.Trainer(0)
    yield t
    t.close()


def _three_ways(tr, corpus, vocab, lockstep=-1, **opts):
    tr.set_option("lockstep", lockstep)
    try:
        return S._three_ways(tr, corpus, vocab, **opts)
    finally:
        tr.set_option("lockstep", -1)


@pytest.mark.parametrize("lockstep", [-1, 0])
def test_runs_ending_at_a_tile_edge(tr, lockstep):
    """Runs of 2 .. 5 of a member's token whose last token sits at slot 511 of a tile, at slot 0 and at slot 1 of the
    next: the tile before then ends on a partial run, which the list pass takes from the register."""
    c = S._Corpus()
    tile = 3
    for end in (511, 512, 513):
        for length in (2, 3, 4, 5):
            c.put(tile, end - length + 1, [201 + length % 2] * length)
            tile += 4
    c.finish([(201, 201), (202, 202), (204, 205)], 40, tile)
    _three_ways(tr, c, 256 + 6, lockstep=lockstep)


def test_runs_across_full_tiles(tr):
    """Runs of 600, 601, 1,100, 1,101, 1,700 and 1,701 equal bytes: the tile behind a run's last full tile walks back
    across one, two and three tiles that are one whole run each, to the tile where the run began (a partial run there,
    or -- the run started at slot 0 -- another token).  Four members at one count; 13.9 M bytes keep 1,701 pairs rare."""
    c = S._Corpus(362)
    c.put(20, 0, [201] * 1700)          # tiles 20 - 22 full, 164 in tile 23
    c.put(40, 0, [202] * 1100)          # two full tiles
    c.put(50, 400, [202] * 601)         # 112, one full tile, 1
    c.put(60, 511, [203] * 1101)        # 1, two full tiles, 76
    c.put(70, 0, [203] * 600)           # one full tile
    c.put(80, 300, [204] * 1701)        # 212, two full tiles, 465
    c.finish([(201, 201), (202, 202), (203, 203), (204, 204)], 1700, 90)
    res = _three_ways(tr, c, 256 + 7, count=False)
    assert len([1 for a, b in res[1][1] if a == b]) >= 4


@pytest.mark.parametrize("barrier", [0, 1])
def test_chunk_ends_at_long_runs(tr, barrier):
    """Runs of 1,100 with a chunk end inside (the token that ends the chunk differs raw: the walk stops there), right
    before and right behind the run, with the end bit (0) and with barrier slots (1)."""
    c = S._Corpus(236)
    at = c.put(20, 0, [201] * 1100)
    c.cuts.append(at + 700)             # inside, in the second full tile
    at = c.put(30, 0, [202] * 1100)
    c.cuts.append(at)                   # right before the run
    at = c.put(40, 0, [203] * 1100)
    c.cuts.append(at + 1100)            # right behind it
    at = c.put(50, 200, [204] * 1100)
    c.cuts.append(at + 312)             # at a tile edge inside the run
    c.finish([(201, 201), (202, 202), (203, 203), (204, 204)], 1100, 60)
    _three_ways(tr, c, 256 + 7, count=False, chunk_barrier=barrier)


def test_sixteen_members_with_full_tiles(tr):
    """16 (kTTMax) members in one batch, each with one run of 585 .. 600 that starts at a slot of its own, so that every
    member's run makes one tile a whole run of it."""
    c = S._Corpus(128)
    members = list(range(200, 216))
    for i, t in enumerate(members):
        c.put(10 + 4 * i, (i * 37) % 500, [t] * (585 + i))
    c.finish([(t, t) for t in members], 600, 80)
    res = _three_ways(tr, c, 256 + 19, count=False, lockstep=0)
    assert len([1 for a, b in res[1][1] if a == b]) >= 16


def test_abandoned_split_pass_runs_at_edges(tr):
    """The construction of test_gpu_tt_split.test_abandoned_split_pass (see there for how the selection is brought to
    pass a candidate over and validation to abandon the pass), with the members' runs of 4 and 5 ending at slots 511, 512
    and 513: k_rewrite_marked<TT> rewrites the marked tiles of the kept prefix with the run scan skipped, and takes the
    run before a tile as the list pass did.  (At these counts no member's run fills a tile: the walk across full tiles
    under k_rewrite_marked is the same function the list pass's cases above exercise.)"""
    c = S._Corpus(80)
    tile = 3
    for t, length in ((201, 5), (202, 4)):
        for end in (300, 511, 512, 513, 514):
            c.put(tile, end - length + 1, [t] * length)
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


def _edge_runs(c, n_edges, members):
    for tile in range(n_edges):
        c.put(tile, 511, [members[tile % len(members)]] * 2)


@pytest.mark.parametrize("lockstep", [-1, 0])
def test_list_far_longer_than_the_last(tr, lockstep):
    """The first split pass lists a handful of tiles (one member, its pairs in two tiles), a later one 1,121 of the 1,357
    (16 members, a run of two across every edge): nothing the list pass uses may be left over from the list before."""
    c = S._Corpus(18)
    members = list(range(200, 216))
    _edge_runs(c, 1120, members)
    assert all(c.count(t, t) == 70 for t in members)
    # (the 16 wait for the later pass: each depends on a pair (x, t) of the first level, which ends in its token)
    tile = c.level([(220, 220)] + [(221 + i, t) for i, t in enumerate(members)], 80, 1130)
    c.level([S.DECOY], 81, tile + 4)
    assert 82 * 8192 < len(c.data)
    res = _three_ways(tr, c, 256 + 36, count=False, lockstep=lockstep)
    seqs = res[1][0]
    per_pass = [b[3] - a[3] for a, b in zip([(0, 0, 0, 0, 0)] + seqs, seqs) if b[2] > a[2]]
    assert len(per_pass) >= 2 and per_pass[0] <= 8 and max(per_pass[1:]) >= 1121, (seqs, per_pass)


def test_list_far_shorter_than_the_last(tr):
    """The other way round: 1,121 tiles listed first, a handful later.  ((238, 239) keeps (220, 220) company: a pair
    that is selected alone is merged by k_merge, not by a fused pass.)"""
    c = S._Corpus(16)
    members = list(range(200, 216))
    _edge_runs(c, 1120, members)
    tile = c.level([(221, 220)], 70, 1130)       # ((220, 220) depends on it, and waits)
    tile = c.level([(220, 220), (238, 239)], 50, tile + 2)
    c.level([S.DECOY], 71, tile + 4)
    assert 72 * 8192 < len(c.data)
    res = _three_ways(tr, c, 256 + 22, count=False)
    seqs = res[1][0]
    per_pass = [b[3] - a[3] for a, b in zip([(0, 0, 0, 0, 0)] + seqs, seqs) if b[2] > a[2]]
    assert len(per_pass) >= 2 and per_pass[0] >= 1121 and min(per_pass[1:]) <= 8, (seqs, per_pass)


def test_frequent_pair_batch_keeps_the_scan(tr):
    """Random bytes over three symbols: every batch with a (t,t) member is the frequent-pair instantiation's, which never
    splits -- the run scan runs and run_in is read as ever, with the route forced on."""
    rng = np.random.default_rng(11)
    data = rng.integers(97, 100, 1 << 16).astype(np.uint8)
    data[1000:2300] = 97
    want_m, want_c = O.train(data, 256 + 40)
    for k, v in dict(S.OPTS, fused_min=2, tt_split=1).items():
        tr.set_option(k, v)
    try:
        got_m, got_c, stats = tr.train_lexical(data, 256 + 40)
    finally:
        for k, v in S.OPTS.items():
            tr.set_option(k, v)
    assert got_m.tolist() == want_m.tolist() and got_c.tolist() == want_c.tolist()
    assert any(a == b for a, b in got_m.tolist())
    assert stats["n_tt_split"] == 0 and stats["tt_deferred_tiles"] == 0, stats
