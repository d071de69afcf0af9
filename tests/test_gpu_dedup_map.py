"""Deduper.unique_of() (option "map" of csrc/dedup.hip): for every chunk the deduper kept, the unique chunk that has its
bytes -- against the Python dedup of tests/dedup_cases.py, through both entry points, with the full hash and with
"hash_bits" 4 and 0.  Without the option the deduper allocates and reports what it did before."""
import numpy as np
import pytest

import mbpe
import dedup_cases as C
from mbpe import check

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def _case_list():
    """The case list of tests/test_gpu_dedup.py, rebuilt from the same generators."""
    cases = {
        "none": [],
        "one": [b"hello"],
        "all-equal": [b"same"] * 700,
        "all-distinct": C.distinct_chunks(600),
        "one-byte": [bytes([97 + (i * 7) % 5]) for i in range(900)],
        "many-duplicates": C.random_chunks(1, 20000, 12, 3),
        "two-symbols": C.random_chunks(2, 20000, 12, 2),
        "four-symbols": C.random_chunks(3, 20000, 12, 4),
        "long": C.long_chunks(),
    }
    for k in (1, 4, 1025):
        for d in (-1, 0, 1):
            cases["edge-%d%+d" % (k, d)] = C.edge_chunks(k + d, 16 * k + d)
    return cases


def unique_of(chunks, max_chunk_bytes=C.MAX_CHUNK_BYTES):
    """The map that goes with dedup_cases.dedup: the index among the unique chunks of every chunk."""
    index, out, n = {}, [], 0
    for c in chunks:
        j = index.get(c) if len(c) <= max_chunk_bytes else None
        if j is None:
            j = n
            n += 1
            if len(c) <= max_chunk_bytes:
                index[c] = j
        out.append(j)
    return out


CASES = _case_list()
WANT = {name: (C.dedup(chunks), unique_of(chunks)) for name, chunks in CASES.items()}     # once, shared, never changed


def _check(dd, dev, chunks, want):
    (want_u, _, want_f), want_map = want
    got = dd.unique_of()
    assert got.dtype == np.uint32 and got.tolist() == want_map
    # it names a chunk with the same bytes, and a first occurrence names itself
    assert all(want_u[j] == c for j, c in zip(want_map, chunks))
    assert [want_map[f] for f in want_f] == list(range(len(want_u)))
    ptr, n = dd.map_device()
    assert n == len(chunks) and ptr
    if n:
        view = check._as_tensor(torch, ptr, 4 * n, torch.uint8, dev).cpu().numpy().view(np.uint32)
        assert view.tolist() == want_map


@pytest.mark.parametrize("hash_bits", [64, 4, 0])
@pytest.mark.parametrize("name", sorted(CASES))
def test_unique_of_against_python_dedup(dev, name, hash_bits):
    chunks = CASES[name]
    data, off = C.join(chunks)
    with mbpe.Deduper(0) as dd:
        dd.set_option("map", 1)
        dd.set_option("hash_bits", hash_bits)
        assert dd.chunks(data, off) == (len(WANT[name][0][0]), sum(len(c) for c in WANT[name][0][0]))
        _check(dd, dev, chunks, WANT[name])
        text = torch.from_numpy(np.concatenate([data, np.zeros(16, dtype=np.uint8)])).to(dev)
        mask = torch.from_numpy(C.end_mask(off, len(data))).to(dev)
        dd.chunks_endmask(text.data_ptr(), len(data), mask.data_ptr())
        _check(dd, dev, chunks, WANT[name])


def test_empty_chunks_stay_out(dev):
    chunks = [b"ab", b"", b"", b"cd", b"ab", b"", b"e", b"cd"]
    data = np.frombuffer(b"".join(chunks), dtype=np.uint8)
    off = np.concatenate([[0], np.cumsum([len(c) for c in chunks])]).astype(np.uint64)
    with mbpe.Deduper(0) as dd:
        dd.set_option("map", 1)
        assert dd.chunks(data, off) == (3, 5)
        assert dd.unique_of().tolist() == [0, 1, 0, 2, 1]


def test_long_chunks_are_their_own(dev):
    chunks = C.long_chunks()
    data, off = C.join(chunks)
    with mbpe.Deduper(0) as dd:
        dd.set_option("map", 1)
        dd.chunks(data, off)
        assert dd.unique_of().tolist() == unique_of(chunks)
        dd.set_option("max_chunk_bytes", 8192)
        dd.chunks(data, off)
        assert dd.unique_of().tolist() == unique_of(chunks, 8192)
        assert len(set(unique_of(chunks, 8192))) < len(set(unique_of(chunks)))


def test_without_the_option_nothing_changes(dev):
    data, off = C.join(CASES["many-duplicates"])
    with mbpe.Deduper(0) as plain, mbpe.Deduper(0) as mapped:
        mapped.set_option("map", 1)
        assert plain.chunks(data, off) == mapped.chunks(data, off)
        assert mapped.alloc_count() == plain.alloc_count() + 1            # the map, 4 B per chunk, and nothing else
        a, b = plain.get(), mapped.get()
        assert a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:]))
        for call in (plain.unique_of, plain.map_device):
            with pytest.raises(mbpe.MbpeError) as e:
                call()
            assert e.value.code == mbpe.ERR_STATE
        # switched off again: the next result has no map, and a repeat allocates nothing
        before = mapped.alloc_count()
        mapped.chunks(data, off)
        assert mapped.alloc_count() == before
        mapped.set_option("map", 0)
        mapped.chunks(data, off)
        with pytest.raises(mbpe.MbpeError) as e:
            mapped.unique_of()
        assert e.value.code == mbpe.ERR_STATE
        for bad in (2, -1):
            with pytest.raises(mbpe.MbpeError) as e:
                mapped.set_option("map", bad)
            assert e.value.code == mbpe.ERR_ARG
    with mbpe.Deduper(0) as fresh:
        with pytest.raises(mbpe.MbpeError) as e:
            fresh.unique_of()
        assert e.value.code == mbpe.ERR_STATE
