"""mbpe.Deduper (csrc/dedup.hip) against the Python dedup of tests/dedup_cases.py: unique text, end mask, weights and
first_chunk must be equal, with the full hash and with "hash_bits" 4 and 0, where distinct chunks share a hash (and, at
0, one probe sequence) so that only the byte compare tells them apart."""
import numpy as np
import pytest

import mbpe
import oracle as O
import dedup_cases as C
from conftest import read_data
from mbpe import check

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def dd():
    d = mbpe.Deduper(0)
    yield d
    d.close()


def _case_list():
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
    for k in (1, 4, 1025):            # 16 k - 1, 16 k, 16 k + 1 bytes; 1,025 x 16 bytes pass a 16-KiB tile of the mask
        for d in (-1, 0, 1):
            cases["edge-%d%+d" % (k, d)] = C.edge_chunks(k + d, 16 * k + d)
    return cases


CASES = _case_list()
WANT = {name: C.dedup(chunks) for name, chunks in CASES.items()}      # computed once, shared, never changed


def _device_bytes(ptr, n, dev):
    return check._as_tensor(torch, ptr, n, torch.uint8, dev).cpu().numpy()


def _equal(dd, dev, chunks, want, counts):
    want_u, want_w, want_f = want
    nu, nb = counts
    assert (nu, nb) == (len(want_u), sum(len(c) for c in want_u))
    text_out, off_out, w, f = dd.get()
    want_text, want_off = C.join(want_u)
    assert text_out == want_text.tobytes()
    assert off_out.tolist() == want_off.tolist()
    assert w.tolist() == want_w and f.tolist() == want_f
    assert int(w.astype(np.uint64).sum()) == len(chunks)
    # the device views: the same text, and the end mask in the layout the trainer reads, nothing set beyond
    t_ptr, m_ptr, w_ptr, f_ptr = dd.result()
    assert t_ptr and m_ptr and w_ptr and f_ptr
    assert _device_bytes(t_ptr, nb, dev).tobytes() == text_out
    n_mask = mbpe.Splitter.mask_bytes(nb)
    assert np.array_equal(_device_bytes(m_ptr, n_mask, dev), C.end_mask(want_off, nb))
    assert _device_bytes(w_ptr, 4 * nu, dev).view(np.uint32).tolist() == want_w


@pytest.mark.parametrize("hash_bits", [64, 4, 0])
@pytest.mark.parametrize("name", sorted(CASES))
def test_against_python_dedup(dd, dev, name, hash_bits):
    chunks = CASES[name]
    data, off = C.join(chunks)
    dd.set_option("hash_bits", hash_bits)
    try:
        _equal(dd, dev, chunks, WANT[name], dd.chunks(data, off))
        # the same chunks as device text with an end mask
        text = torch.from_numpy(np.concatenate([data, np.zeros(16, dtype=np.uint8)])).to(dev)
        mask = torch.from_numpy(C.end_mask(off, len(data))).to(dev)
        _equal(dd, dev, chunks, WANT[name], dd.chunks_endmask(text.data_ptr(), len(data), mask.data_ptr()))
    finally:
        dd.set_option("hash_bits", 64)


def test_long_chunks_pass_through(dd):
    chunks = CASES["long"]
    u, w, f = WANT["long"]
    longest = max(len(c) for c in chunks)
    assert longest == C.MAX_CHUNK_BYTES + 1
    assert [len(c) for c in u].count(longest) == 2 and all(w[i] == 1 for i, c in enumerate(u) if len(c) == longest)
    assert [len(c) for c in u].count(C.MAX_CHUNK_BYTES) == 1 and [len(c) for c in u].count(C.MAX_CHUNK_BYTES - 1) == 1
    # a lower limit: what passed as one class before now appears twice
    data, off = C.join(chunks)
    dd.set_option("max_chunk_bytes", C.MAX_CHUNK_BYTES - 1)
    try:
        nu, _ = dd.chunks(data, off)
        want = C.dedup(chunks, C.MAX_CHUNK_BYTES - 1)
        assert nu == len(want[0]) == len(u) + 1
        assert dd.get()[2].tolist() == want[1]
    finally:
        dd.set_option("max_chunk_bytes", C.MAX_CHUNK_BYTES)


def test_empty_chunks_vanish_and_first_chunk_counts_them(dd):
    chunks = [b"ab", b"", b"", b"cd", b"ab", b"", b"e"]
    data = np.frombuffer(b"".join(chunks), dtype=np.uint8)
    off = np.concatenate([[0], np.cumsum([len(c) for c in chunks])]).astype(np.uint64)
    assert dd.chunks(data, off) == (3, 5)
    text, u_off, w, f = dd.get()
    assert text == b"abcde" and u_off.tolist() == [0, 2, 4, 5] and w.tolist() == [2, 1, 1] and f.tolist() == [0, 3, 6]


@pytest.mark.parametrize("encoder", ["gpt2", "gpt4"])
def test_taylorswift_after_the_device_split(dd, dev, encoder):
    data = read_data("taylorswift.txt")
    pattern = O.GPT4_SPLIT_PATTERN if encoder == "gpt4" else O.GPT2_SPLIT_PATTERN
    chunks = C.chunks_of(data, mbpe.presplit(pattern, data))
    with mbpe.Splitter(pattern) as sp:
        assert sp.split(data, offsets=False) == len(chunks)
        m_ptr, _, t_ptr = sp.endmask()
        counts = dd.chunks_endmask(t_ptr, len(data), m_ptr)
        _equal(dd, dev, chunks, C.dedup(chunks), counts)
    print(encoder, len(chunks), "chunks", counts, "unique chunks / bytes,", dd.kernel_ms(), "ms")


def test_repeat_call_allocates_nothing(dd):
    data, off = C.join(CASES["many-duplicates"])
    dd.chunks(data, off)
    before = dd.alloc_count()
    first = dd.get()
    dd.chunks(data, off)
    small, small_off = C.join(CASES["one-byte"])
    dd.chunks(small, small_off)
    dd.chunks(data, off)
    assert dd.alloc_count() == before
    again = dd.get()
    assert first[0] == again[0] and all(np.array_equal(a, b) for a, b in zip(first[1:], again[1:]))
    assert dd.kernel_ms() > 0


def test_get_with_caps_too_small_and_bad_arguments(dd):
    data, off = C.join(CASES["all-distinct"])
    nu, nb = dd.chunks(data, off)
    for kw in ({"cap_bytes": nb - 1}, {"cap_chunks": nu - 1}, {"cap_bytes": 0, "cap_chunks": 0}):
        with pytest.raises(mbpe.MbpeError) as e:
            dd.get(**kw)
        assert e.value.code == mbpe.ERR_ARG
    assert dd.get()[2].tolist() == [1] * nu
    for bad in (np.array([1, 4], dtype=np.uint64), np.array([0, 3, 2, len(data)], dtype=np.uint64),
                np.array([0, len(data) - 1], dtype=np.uint64)):
        with pytest.raises(mbpe.MbpeError) as e:
            dd.chunks(data, bad)
        assert e.value.code == mbpe.ERR_ARG
    for name, value in (("hash_bits", 65), ("hash_bits", -1), ("max_chunk_bytes", -1), ("no_such_option", 1)):
        with pytest.raises(mbpe.MbpeError) as e:
            dd.set_option(name, value)
        assert e.value.code == mbpe.ERR_ARG
    with mbpe.Deduper(0) as fresh:
        with pytest.raises(mbpe.MbpeError) as e:
            fresh.result()
        assert e.value.code == mbpe.ERR_STATE
