"""mbpe.WordCount (csrc/wordcount.hip) against one Python dedup of the pieces' chunk lists laid end to end
(tests/dedup_cases.py): text, offsets, weights and first_chunk must be equal, whatever the cut, with the full hash and
with "hash_bits" 4 and 0, across table rebuilds, with repeats, and up to the 2^31 limit of a weight."""
import numpy as np
import pytest

import mbpe
import oracle as O
import dedup_cases as C
import wordcount_cases as W
from conftest import read_data
from mbpe import check

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


@pytest.fixture
def wc():
    w = mbpe.WordCount(0)
    yield w
    w.close()


def _device_bytes(ptr, n, dev):
    return check._as_tensor(torch, ptr, n, torch.uint8, dev).cpu().numpy()


def _equal(wc, want, n_chunks_total=None, dev=None):
    want_u, want_w, want_f = want
    want_text, want_off = C.join(want_u)
    text, off, w, f = wc.get()
    assert (wc.n_unique, wc.n_unique_bytes) == (len(want_u), len(want_text))
    assert text == want_text.tobytes()
    assert off.tolist() == want_off.tolist()
    assert w.tolist() == want_w and f.tolist() == want_f
    st = wc.stats()
    assert (st["n_unique"], st["n_unique_bytes"]) == (len(want_u), len(want_text))
    if n_chunks_total is not None:
        assert st["n_chunks_total"] == n_chunks_total == sum(want_w)
    if dev is not None:
        # the device views: the same text, the end mask in the layout the trainer reads with nothing set beyond, u32 weights
        t_ptr, m_ptr, w_ptr, f_ptr = wc.result()
        assert t_ptr and m_ptr and w_ptr and f_ptr
        nb, nu = len(want_text), len(want_u)
        assert _device_bytes(t_ptr, nb, dev).tobytes() == text
        assert np.array_equal(_device_bytes(m_ptr, mbpe.Splitter.mask_bytes(nb), dev), C.end_mask(want_off, nb))
        assert _device_bytes(w_ptr, 4 * nu, dev).view(np.uint32).tolist() == want_w
        assert _device_bytes(f_ptr, 8 * nu, dev).view(np.uint64).tolist() == want_f


def _add_all(wc, pieces, hash_bits=64):
    wc.set_option("hash_bits", hash_bits)
    for p in pieces:
        data, off = C.join(p)
        wc.add(data, off)


@pytest.mark.parametrize("hash_bits", [64, 4, 0])
@pytest.mark.parametrize("n_pieces", [1, 2, 7])
@pytest.mark.parametrize("seed", range(3))
def test_random_chunks_in_pieces(wc, dev, seed, n_pieces, hash_bits):
    rng = np.random.default_rng(40 + seed)
    chunks = C.random_chunks(seed, int(rng.integers(50, 1500)), 12, int(rng.integers(1, 5)))
    pieces = W.cut_list(chunks, n_pieces)
    pieces.insert(len(pieces) // 2, [])                                   # an empty piece
    pieces.append(max(pieces, key=len))                                   # a piece that only repeats
    pieces.append([b"new-%d" % i for i in range(300)])                    # a piece that is all new
    _add_all(wc, pieces, hash_bits)
    _equal(wc, C.dedup(W.concat(pieces)), len(W.concat(pieces)), dev)
    assert wc.stats()["n_pieces"] == len(pieces)


@pytest.mark.parametrize("hash_bits", [64, 0])
@pytest.mark.parametrize("d", [-1, 0, 1])
def test_alignment_and_mask_word_edges(wc, dev, d, hash_bits):
    chunks = C.edge_chunks(3, 16 * 40 + d)
    pieces = [chunks[0::3], chunks[1::3] + chunks[2::3]]
    _add_all(wc, pieces, hash_bits)
    _equal(wc, C.dedup(W.concat(pieces)), len(chunks), dev)


@pytest.mark.parametrize("hash_bits", [64, 4])
def test_long_chunks_over_two_pieces(wc, dev, hash_bits):
    chunks = C.long_chunks()
    pieces = [chunks[:5], chunks[5:]]
    _add_all(wc, pieces, hash_bits)
    want = C.dedup(chunks)
    assert [len(c) for c in want[0]].count(C.MAX_CHUNK_BYTES + 1) == 2
    _equal(wc, want, len(chunks), dev)


def test_a_lower_max_chunk_bytes_reaches_the_deduper(wc):
    chunks = C.long_chunks()
    wc.set_option("max_chunk_bytes", C.MAX_CHUNK_BYTES - 1)
    _add_all(wc, [chunks[:5], chunks[5:]])
    _equal(wc, C.dedup(chunks, C.MAX_CHUNK_BYTES - 1), len(chunks))
    with pytest.raises(mbpe.MbpeError) as e:
        wc.set_option("max_chunk_bytes", 3)
    assert e.value.code == mbpe.ERR_STATE
    wc.reset()
    wc.set_option("max_chunk_bytes", C.MAX_CHUNK_BYTES)


@pytest.mark.parametrize("hash_bits", [64, 4, 0])
def test_table_rebuilds_keep_the_earlier_entries(wc, dev, hash_bits):
    chunks = C.distinct_chunks(16 + 64 + 256 + 2000)
    pieces = [chunks[0:16], chunks[16:80], chunks[80:336], chunks[336:], chunks[0:16]]
    _add_all(wc, pieces, hash_bits)
    want = C.dedup(W.concat(pieces))
    assert want[1][:17] == [2] * 16 + [1] and len(want[0]) == len(chunks)
    _equal(wc, want, len(chunks) + 16, dev)


def test_host_text_with_empty_chunks(wc):
    first = [b"ab", b"", b"", b"cd", b"ab", b"", b"e"]
    second = [b"", b"e", b"f", b"", b"ab"]
    for p in (first, second):
        data = np.frombuffer(b"".join(p), dtype=np.uint8)
        off = np.concatenate([[0], np.cumsum([len(c) for c in p])]).astype(np.uint64)
        wc.add(data, off)
    text, off, w, f = wc.get()
    # first_chunk still counts the empty chunks: the index in first + second as they were given
    assert text == b"abcdef" and off.tolist() == [0, 2, 4, 5, 6]
    assert w.tolist() == [3, 1, 2, 1] and f.tolist() == [0, 3, 6, 9]
    assert wc.stats()["n_chunks_total"] == 7


def test_device_text(wc, dev):
    pieces = W.cut_list(C.random_chunks(9, 1200, 12, 3), 3)
    keep = []
    for p in pieces:
        data, off = C.join(p)
        text = torch.from_numpy(np.concatenate([data, np.zeros(16, dtype=np.uint8)])).to(dev)
        keep.append(text)
        wc.add(None, off, text_ptr=text.data_ptr(), n_bytes=len(data))
    _equal(wc, C.dedup(W.concat(pieces)), 1200, dev)


def test_after_the_device_split(wc, dev):
    data = read_data("small.txt")
    pieces = W.cut_text(data, 3)
    chunks = []
    with mbpe.Splitter(O.GPT4_SPLIT_PATTERN) as sp:
        for p in pieces:
            here = C.chunks_of(p, mbpe.presplit(O.GPT4_SPLIT_PATTERN, p))
            assert sp.split(p, offsets=False) == len(here)
            m_ptr, _, t_ptr = sp.endmask()
            wc.add_endmask(t_ptr, len(p), m_ptr)
            chunks += here
    _equal(wc, C.dedup(chunks), len(chunks), dev)


def test_repeat(wc, dev):
    pieces = W.cut_list(C.random_chunks(5, 900, 10, 3), 3)
    acc = W.Accumulator()
    for p, rep in zip(pieces, (1, 3, 2)):
        data, off = C.join(p)
        wc.add(data, off, repeat=rep)
        acc.add(p, rep)
    _equal(wc, acc.result(), acc.n_chunks_total, dev)
    assert wc.stats() == {"n_pieces": 3, "n_chunks_total": len(pieces[0]) + 3 * len(pieces[1]) + 2 * len(pieces[2]),
                          "n_unique": len(acc.uniq), "n_unique_bytes": sum(len(c) for c in acc.uniq)}
    by_repeat = wc.get()
    # the same as adding the piece `repeat` times: one dedup of the written-out list
    wc.reset()
    for p, rep in zip(pieces, (1, 3, 2)):
        data, off = C.join(p)
        for _ in range(rep):
            wc.add(data, off)
    written_out = wc.get()
    assert by_repeat[0] == written_out[0] and by_repeat[1].tolist() == written_out[1].tolist()
    assert by_repeat[2].tolist() == written_out[2].tolist()
    assert written_out[3].tolist() == C.dedup(pieces[0] + pieces[1] * 3 + pieces[2] * 2)[2] == by_repeat[3].tolist()
    with pytest.raises(mbpe.MbpeError) as e:
        wc.add(*C.join(pieces[0]), repeat=0)
    assert e.value.code == mbpe.ERR_ARG


def test_overflow_is_sticky_until_reset(wc):
    data, off = C.join([b"word"])
    other, other_off = C.join([b"other", b"x"])
    wc.add(data, off, repeat=(1 << 31) - 1)
    wc.add(other, other_off)
    text, _, w, _ = wc.get()
    assert text == b"wordotherx" and w.tolist() == [(1 << 31) - 1, 1, 1]
    assert wc.result()[0]
    wc.add(data, off)                                   # one more occurrence: 2^31
    for call in (wc.result, wc.get):
        with pytest.raises(mbpe.MbpeError) as e:
            call()
        assert e.value.code == mbpe.ERR_OVERFLOW
    wc.add(other, other_off)                            # sticky
    for call in (wc.result, wc.get):
        with pytest.raises(mbpe.MbpeError) as e:
            call()
        assert e.value.code == mbpe.ERR_OVERFLOW
    assert wc.stats()["n_chunks_total"] == (1 << 31) + 4
    wc.reset()
    wc.add(other, other_off)
    _equal(wc, ([b"other", b"x"], [1, 1], [0, 1]), 2)
    # a new chunk whose repeat alone is too much
    wc.add(data, off, repeat=1 << 31)
    with pytest.raises(mbpe.MbpeError) as e:
        wc.get()
    assert e.value.code == mbpe.ERR_OVERFLOW


def test_repeat_add_allocates_nothing_and_reset_repeats_the_result(wc):
    pieces = W.cut_list(C.random_chunks(1, 20000, 12, 3), 4)
    _add_all(wc, pieces)
    first = wc.get()
    wc.result()
    before = wc.alloc_count()
    for p in (pieces[1], pieces[3][:100], pieces[0]):      # no new chunk, none larger than an earlier piece
        data, off = C.join(p)
        wc.add(data, off)
    wc.result()
    assert wc.alloc_count() == before
    assert wc.kernel_ms() > 0
    wc.reset()
    assert wc.stats() == {"n_pieces": 0, "n_chunks_total": 0, "n_unique": 0, "n_unique_bytes": 0}
    _add_all(wc, pieces)
    again = wc.get()
    assert wc.alloc_count() == before
    assert first[0] == again[0] and all(np.array_equal(a, b) for a, b in zip(first[1:], again[1:]))
    _equal(wc, C.dedup(W.concat(pieces)), 20000)


def test_nothing_added_and_bad_arguments(wc, dev):
    _equal(wc, ([], [], []), 0, dev)
    data, off = C.join(C.distinct_chunks(10))
    for bad in (np.array([1, 4], dtype=np.uint64), np.array([0, 3, 2, len(data)], dtype=np.uint64)):
        with pytest.raises(mbpe.MbpeError) as e:
            wc.add(data, bad)
        assert e.value.code == mbpe.ERR_ARG
    assert wc.stats()["n_pieces"] == 0
    for name, value in (("hash_bits", 65), ("max_chunk_bytes", -1), ("map", 1)):
        with pytest.raises(mbpe.MbpeError) as e:
            wc.set_option(name, value)
        assert e.value.code == mbpe.ERR_ARG
