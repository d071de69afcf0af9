"""mbpe.WordCount.export / merge (csrc/wordcount.hip) against the Python rule of tests/wordcount_merge_cases.py: tables
counted in separate objects and merged -- by blob, by object, as a chain and as a tree -- must be, bit for bit, the
table of counting all pieces into one object: text, offsets, weights, first_chunk, statistics, device views, and the
exported blob itself, which carries the u64 weights, chunk_base and n_pieces.  A blob that breaks a rule is refused
with the target unchanged."""
import struct

import numpy as np
import pytest

import mbpe
import dedup_cases as C
import wordcount_cases as W
import wordcount_merge_cases as M
from test_gpu_wordcount import _equal

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


@pytest.fixture
def made():
    """-> make(): a fresh WordCount that is closed after the test."""
    objs = []

    def make(hash_bits=64, max_chunk_bytes=None):
        w = mbpe.WordCount(0)
        objs.append(w)
        w.set_option("hash_bits", hash_bits)
        if max_chunk_bytes is not None:
            w.set_option("max_chunk_bytes", max_chunk_bytes)
        return w

    yield make
    for w in objs:
        w.close()


def _count(make, pieces, hash_bits=64, max_chunk_bytes=None, repeats=None):
    w = make(hash_bits, max_chunk_bytes)
    for k, p in enumerate(pieces):
        data, off = C.join(p)
        w.add(data, off, repeat=1 if repeats is None else repeats[k])
    return w


def _full(wc, acc, dev=None):
    """Everything the statement covers: the host copies, the statistics, the device views, and the blob byte for byte."""
    _equal(wc, acc.result(), acc.n_chunks_total, dev)
    assert wc.stats()["n_pieces"] == acc.n_pieces
    assert wc.export() == M.blob_of(acc)


def _flat(groups):
    """The pieces of all groups in order, the empty ones included."""
    return [p for g in groups for p in g]


def _pieces(seed):
    rng = np.random.default_rng(90 + seed)
    chunks = C.random_chunks(seed, int(rng.integers(300, 2000)), 12, int(rng.integers(1, 5)))
    pieces = W.cut_list(chunks, 14)
    pieces.insert(5, [])
    return pieces


@pytest.mark.parametrize("hash_bits", [64, 4, 0])
@pytest.mark.parametrize("n_tables", [2, 3, 7])
@pytest.mark.parametrize("seed", range(2))
def test_random_tables_merged_by_blob_in_order(made, dev, seed, n_tables, hash_bits):
    pieces = _pieces(seed)
    groups = M.groups(pieces, n_tables)
    groups.insert(1, [])                                                   # an empty table in the middle
    groups.append([max(pieces, key=len)])                                  # one that only repeats the target's chunks
    groups.append([[b"new-%d" % i for i in range(300)]])                   # one that is all new
    blobs = [_count(made, g, hash_bits).export() for g in groups]
    assert [M.blob_of(M.count(g)) for g in groups] == blobs
    target = made(hash_bits)                                               # an empty table on the target's side
    for b in blobs:
        target.merge(b)
    whole = M.count(_flat(groups))
    assert whole.result() == C.dedup(W.concat(_flat(groups)))
    _full(target, whole, dev)
    # the same by one object counting all pieces
    _full(_count(made, _flat(groups), hash_bits), whole)


@pytest.mark.parametrize("hash_bits", [64, 0])
def test_chain_tree_blob_and_object_merges_are_identical(made, dev, hash_bits):
    pieces = _pieces(7)
    groups = M.groups(pieces, 3)
    whole = M.count(pieces)
    # chain by object: (T0 + T1) + T2
    t = [_count(made, g, hash_bits) for g in groups]
    t[0].merge(t[1])
    t[0].merge(t[2])
    _full(t[0], whole, dev)
    _full(t[1], M.count(groups[1]), dev)                                   # `other` is left unchanged
    # tree by object: T0 + (T1 + T2)
    u = [_count(made, g, hash_bits) for g in groups]
    u[1].merge(u[2])
    u[0].merge(u[1])
    _full(u[0], whole, dev)
    # tree by blob
    v = [_count(made, g, hash_bits) for g in groups]
    v[1].merge(v[2].export())
    v[0].merge(v[1].export())
    _full(v[0], whole, dev)
    assert t[0].export() == u[0].export() == v[0].export()


def test_import_into_an_empty_object_reproduces_the_blob(made, dev):
    pieces = _pieces(3)
    blob = _count(made, pieces, repeats=[1 + k % 3 for k in range(len(pieces))]).export()
    w = made()
    assert w.merge(blob) == (w.n_unique, w.n_unique_bytes)
    assert w.export() == blob
    _full(w, M.count(pieces, repeats=[1 + k % 3 for k in range(len(pieces))]), dev)
    empty = made().export()
    assert len(empty) == 64 and made().merge(empty) == (0, 0)


@pytest.mark.parametrize("hash_bits", [64, 4, 0])
def test_a_merge_that_rebuilds_the_table_keeps_the_earlier_entries(made, dev, hash_bits):
    chunks = C.distinct_chunks(16 + 2336)
    groups = [[chunks[:16]], [chunks[16:80], chunks[80:336], chunks[336:]], [chunks[:16], chunks[2000:2010]]]
    target = _count(made, groups[0], hash_bits)
    target.merge(_count(made, groups[1], hash_bits).export())
    target.merge(_count(made, groups[2], hash_bits))                       # the earlier entries are still found
    whole = M.count(_flat(groups))
    assert whole.weights[:17] == [2] * 16 + [1] and len(whole.uniq) == len(chunks)
    _full(target, whole, dev)


@pytest.mark.parametrize("by_blob", [True, False], ids=["blob", "object"])
@pytest.mark.parametrize("d", [-1, 0, 1])
def test_alignment_phases_of_the_16_byte_copy(made, dev, d, by_blob):
    chunks = C.edge_chunks(3, 16 * 40 + d)
    groups = [[chunks[0::3]], [chunks[1::3] + chunks[2::3]]]
    target, other = (_count(made, g) for g in groups)
    target.merge(other.export() if by_blob else other)
    whole = M.count(_flat(groups))
    assert whole.result() == C.dedup(W.concat(_flat(groups)))
    _full(target, whole, dev)


@pytest.mark.parametrize("max_chunk_bytes", [None, C.MAX_CHUNK_BYTES - 1])
@pytest.mark.parametrize("hash_bits", [64, 4])
def test_long_chunks_over_two_tables(made, dev, hash_bits, max_chunk_bytes):
    chunks = C.long_chunks()
    limit = C.MAX_CHUNK_BYTES if max_chunk_bytes is None else max_chunk_bytes
    target = _count(made, [chunks[:5]], hash_bits, max_chunk_bytes)
    target.merge(_count(made, [chunks[5:]], hash_bits, max_chunk_bytes).export())
    whole = M.count([chunks[:5], chunks[5:]], limit)
    assert whole.result() == C.dedup(chunks, limit)
    assert [len(c) for c in whole.uniq].count(C.MAX_CHUNK_BYTES + 1) == 2          # duplicates stay separate
    _full(target, whole, dev)


def test_chunk_base_travels_with_empty_chunks(made):
    first = [b"ab", b"", b"", b"cd", b"ab", b"", b"e"]
    second = [b"", b"e", b"f", b"", b"ab"]
    objs = []
    for p in (first, second):
        w = made()
        data = np.frombuffer(b"".join(p), dtype=np.uint8)
        off = np.concatenate([[0], np.cumsum([len(c) for c in p])]).astype(np.uint64)
        w.add(data, off)
        objs.append(w)
    by_blob = made()
    by_blob.merge(objs[0].export())
    by_blob.merge(objs[1].export())
    objs[0].merge(objs[1])
    for w in (by_blob, objs[0]):
        text, off, wt, f = w.get()
        # first_chunk still counts the empty chunks of both lists: chunk_base is 7 after the first, 12 after both
        assert text == b"abcdef" and off.tolist() == [0, 2, 4, 5, 6]
        assert wt.tolist() == [3, 1, 2, 1] and f.tolist() == [0, 3, 6, 9]
        assert w.stats()["n_chunks_total"] == 7 and w.stats()["n_pieces"] == 2
        assert struct.unpack_from("<II7Q", w.export())[2:] == (256, 4, 6, 2, 7, 12, 0)


def test_repeats_then_merge_then_further_adds(made, dev):
    pieces = W.cut_list(C.random_chunks(5, 1200, 10, 3), 6)
    reps = [1, 3, 2, 1, 4, 2]
    target = _count(made, pieces[:2], repeats=reps[:2])
    target.merge(_count(made, pieces[2:4], repeats=reps[2:4]).export())
    for p, r in zip(pieces[4:], reps[4:]):
        data, off = C.join(p)
        target.add(data, off, repeat=r)
    _full(target, M.count(pieces, repeats=reps), dev)
    # and the rule itself: two accumulators merged, then added to
    acc = M.count(pieces[:2], repeats=reps[:2])
    acc.merge(M.count(pieces[2:4], repeats=reps[2:4]))
    for p, r in zip(pieces[4:], reps[4:]):
        acc.add(p, r)
    _full(target, acc)


@pytest.mark.parametrize("by_blob", [True, False], ids=["blob", "object"])
def test_overflow_is_sticky_until_reset(made, by_blob):
    data, off = C.join([b"word"])
    other, other_off = C.join([b"other", b"x"])
    target, once = made(), made()
    target.add(data, off, repeat=(1 << 31) - 1)
    target.add(other, other_off)
    once.add(data, off)
    assert target.get()[2].tolist() == [(1 << 31) - 1, 1, 1] and len(target.export()) == 64 + 72 + 16
    target.merge(once.export() if by_blob else once)                      # one more occurrence: 2^31
    for again in range(2):
        for call in (target.result, target.get, target.export):
            with pytest.raises(mbpe.MbpeError) as e:
                call()
            assert e.value.code == mbpe.ERR_OVERFLOW
        target.add(other, other_off)                                      # sticky
    assert target.stats()["n_chunks_total"] == (1 << 31) + 6
    assert once.get()[2].tolist() == [1]
    if not by_blob:                                                       # an overflowed table is no source either
        with pytest.raises(mbpe.MbpeError) as e:
            once.merge(target)
        assert e.value.code == mbpe.ERR_OVERFLOW
    target.reset()
    target.merge(once.export())
    _equal(target, ([b"word"], [1], [0]), 1)


def test_refusals_leave_the_table_unchanged(made, dev):
    mine = [C.distinct_chunks(40)[::2] * 2, [b"own-%d" % i for i in range(50)]]
    target = _count(made, mine)
    source = M.count([C.distinct_chunks(40), [b"y" * 300, b"y" * 300]])
    acc = M.count(mine)
    before = target.export()
    bad = M.corrupt_blobs(source)
    assert sorted(bad) == ["a hashed chunk twice", "an end out of order", "bad magic", "first_chunk out of order",
                           "other max_chunk_bytes", "truncated", "weight 0", "weights' sum"]
    for name, blob in bad.items():
        with pytest.raises(mbpe.MbpeError) as e:
            target.merge(blob)
        assert e.value.code == mbpe.ERR_ARG, name
        _full(target, acc, dev)
        assert target.export() == before, name
    with pytest.raises(mbpe.MbpeError) as e:
        target.merge(target)
    assert e.value.code == mbpe.ERR_ARG
    other = made(max_chunk_bytes=C.MAX_CHUNK_BYTES - 1)
    with pytest.raises(mbpe.MbpeError) as e:
        target.merge(other)                                               # the options differ
    assert e.value.code == mbpe.ERR_ARG
    _full(target, acc, dev)
    # the blob that breaks no rule is taken
    target.merge(M.blob_of(source))
    acc.merge(source)
    _full(target, acc, dev)


def test_kernel_ms_and_a_second_merge_allocates_nothing(made):
    pieces = W.cut_list(C.random_chunks(1, 20000, 12, 3), 4)
    target = _count(made, pieces)
    blob = _count(made, [pieces[1], pieces[3][:100]]).export()            # only chunks the target has
    target.merge(blob)
    assert target.kernel_ms() > 0
    target.result()
    before = target.alloc_count()
    target.merge(blob)
    target.result()
    assert target.alloc_count() == before
    assert target.kernel_ms() > 0
    acc = M.count(pieces)
    acc.merge(M.count([pieces[1], pieces[3][:100]]))
    acc.merge(M.count([pieces[1], pieces[3][:100]]))
    _full(target, acc)
