"""GPU tests at the 2^31 / 2^32 limits of a design that counts pairs in 32-bit bins and positions in 64 bits.

The pair-count scan adds every workgroup's histogram into 65,536 global u32 bins (the last flush two bins per 64-bit
atomic), and a sharded begin sums the ranks' bins in a u32 all-reduce.  A pair that occurs 2^32 times or more then
leaves a small count in its bin -- and a carry of the 64-bit flush can put 1 into the next bin -- which the 2^31 check
of k_table_init cannot see.  The library must report it (ERR_OVERFLOW), not train on it; and just below the limits it
must count, and train, exactly.

Every expected value is exact: closed forms in Python ints, the oracle's counts of one copy of a text times the number
of copies, or counts taken with torch on the device.  The corpora are built on the device in one buffer of the largest
size, whose prefixes are loaded at the different lengths.
"""
import ctypes

import numpy as np
import pytest

import mbpe
import oracle as O
from mbpe import check as C
from conftest import read_data

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

G = 1 << 30
SHARD = 3 * G // 2                       # 1.5 GiB per rank: three of them hold more than 2^32 pairs in all
TEXT_COPIES = 3900                       # shakespeare.txt x 3,900 = 4.35 GB, past 2^32 slots
LADDER = [(1 << 31) - 1, 1 << 31, (1 << 32) - 1, 1 << 32, (1 << 32) + 5]


@pytest.fixture(scope="module")
def dev():
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def buf(dev):
    """One device buffer for every corpus of this file (the largest: three shards of 1.5 GiB)."""
    n = max(3 * SHARD, TEXT_COPIES * len(read_data("shakespeare.txt")), LADDER[-1] + 2) + 64
    b = torch.empty(n, dtype=torch.uint8, device=dev)
    yield b
    del b
    torch.cuda.empty_cache()


def _small_corpus_trains_like_oracle(tr):
    """After an error, the same context trains a small corpus exactly as the oracle does."""
    data = read_data("taylorswift.txt")[:20000]
    want_m, want_c = O.train(data, 256 + 40)
    m, c, _ = tr.train_lexical(data, 256 + 40)
    assert m.tolist() == want_m.tolist() and c.tolist() == want_c.tolist()


LADDER_IDS = ["2^31-1", "2^31", "2^32-1", "2^32", "2^32+5"]


@pytest.mark.parametrize("c", LADDER, ids=LADDER_IDS)
@pytest.mark.parametrize("b", [0x60, 0x61], ids=["low_half", "high_half"])
@pytest.mark.parametrize("chunked", [False, True], ids=["one_chunk", "masked_scan"])
def test_count_ladder(dev, buf, chunked, b, c):
    """The corpus buf[:n] all bytes `b`, so that the pair (b, b) occurs c times: one chunk (n = c + 1,
    k_pair_count_u8_fast) or two chunks cut at 1 MiB (n = c + 2, the masked scan k_pair_count_u8<true>); (b, b) in the
    low (0x60) and in the high (0x61) bin of its 64-bit flush word.  Below 2^32 the table is exact -- (b, b) = c and
    nothing else, not the neighbour (b, b + 1) that a carry of the flush would reach -- and from 2^32 on (at 2^32 the bin
    wraps to 0: the pair vanishes) pair_count_u8 reports it.  train_begin takes only counts that fit 31 bits.  After an
    error the context trains a small corpus exactly like the oracle."""
    n = c + (2 if chunked else 1)
    buf[:n].fill_(b)
    torch.cuda.synchronize()
    bb = (b << 8) | b
    with mbpe.Trainer(0) as tr:
        tr.set_option("chunk_barrier", 0)
        tr.load_corpus_device(buf.data_ptr(), n, [0, 1 << 20, n] if chunked else None, keep=buf)
        if c < 1 << 32:
            got = tr.pair_count_u8()
            assert int(got[bb]) == c and int(got[bb + 1]) == 0
            assert int(got.astype(np.int64).sum()) == c
        else:
            with pytest.raises(mbpe.MbpeError) as e:
                tr.pair_count_u8()
            assert e.value.code == mbpe.ERR_OVERFLOW
            _small_corpus_trains_like_oracle(tr)
            tr.load_corpus_device(buf.data_ptr(), n, [0, 1 << 20, n] if chunked else None, keep=buf)
        if c == (1 << 31) - 1:
            assert tr.train_begin(257) == mbpe.OK
            assert tr.train_steps(1) == 1
            m, cnt = tr.train_result()
            assert m.tolist() == [[b, b]] and cnt.tolist() == [c]
            return
        with pytest.raises(mbpe.MbpeError) as e:
            tr.train_begin(257)
        assert e.value.code == mbpe.ERR_OVERFLOW
        _small_corpus_trains_like_oracle(tr)


def test_masked_scan_just_below_2_pow_32_is_exact(dev, buf):
    """2^32 bytes of one value (its pair: 2^32 - 1 times) and a second chunk of 4 MiB of random bytes that never hold
    it: the table equals the reference in every bin -- a count just below the limit neither carries into its neighbour
    nor trips the check of the sum."""
    b = 0x60
    n_run, n_rand = 1 << 32, 4 << 20
    n = n_run + n_rand
    buf[:n_run].fill_(b)
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    v = torch.randint(0, 255, (n_rand,), dtype=torch.int16, device=dev, generator=g)
    buf[n_run:n] = (v + (v >= b).to(torch.int16)).to(torch.uint8)
    del v
    rand = buf[n_run:n].long()
    want = torch.bincount(rand[:-1] * 256 + rand[1:], minlength=65536).cpu().numpy().astype(np.int64)
    del rand
    assert int(want[(b << 8) | b]) == 0
    want[(b << 8) | b] = n_run - 1                       # the run's pairs; none across the chunk end
    with mbpe.Trainer(0) as tr:
        tr.load_corpus_device(buf.data_ptr(), n, [0, n_run, n], keep=buf)
        got = tr.pair_count_u8().astype(np.int64)
    assert np.array_equal(got, want)


def _run_merges(a, k):
    """2^31 bytes `a`: merge j is (t, t) of the previous run's token, count 2^(31 - j) - 1 (the first: INT_MAX)."""
    toks = [a] + [256 + j for j in range(k - 1)]
    return [[t, t] for t in toks], [(1 << (31 - j)) - 1 for j in range(k)]


@pytest.mark.parametrize("multi_merge", [0, 1])
@pytest.mark.parametrize("mode", [1, 0], ids=["lexical", "first"])
def test_top_of_int32_range_trains(dev, buf, mode, multi_merge):
    """2^31 bytes of 'a', vocab 256 + 31: (a, a) with count INT_MAX, then (256, 256) ... (285, 285), each a single-run
    (t, t) merge over 2^22 tiles, with counts 2^(31 - k) - 1."""
    n, k = 1 << 31, 31
    buf[:n].fill_(ord("a"))
    torch.cuda.synchronize()
    want_m, want_c = _run_merges(ord("a"), k)
    assert want_c[0] == 2 ** 31 - 1 and want_m[-1] == [285, 285]
    with mbpe.Trainer(0) as tr:
        tr.set_option("conflict_resolution", mode)
        tr.set_option("multi_merge", multi_merge)
        tr.load_corpus_device(buf.data_ptr(), n, keep=buf)
        tr.train_begin(256 + k)
        assert tr.train_steps(k) == k
        m, c = tr.train_result()
    assert m.tolist() == want_m and c.tolist() == want_c


_hip = None


def _hipmemcpy():
    global _hip
    if _hip is None:
        _hip = ctypes.CDLL("libamdhip64.so")
        _hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    return _hip.hipMemcpy


def _allreduce_u32(trainers):
    """The collective of the external transport: every rank's exchange buffer summed as u32 (as RCCL sums it)."""
    bufs = [t.exchange_buffer() for t in trainers]
    n = bufs[0][1]
    assert all(x[1] == n for x in bufs)
    total = np.zeros(n, dtype=np.uint32)
    tmp = np.zeros(n, dtype=np.uint32)
    for ptr, _ in bufs:
        assert _hipmemcpy()(tmp.ctypes.data, ptr, n * 4, 2) == 0       # D2H
        total += tmp
    for ptr, _ in bufs:
        assert _hipmemcpy()(ptr, total.ctypes.data, n * 4, 1) == 0     # H2D


def _sharded_begin(buf, n_ranks, shard, vocab):
    """Contexts 0..n_ranks-1 on shards buf[r * shard:(r + 1) * shard] (16-byte aligned), begun up to the exchange."""
    assert shard % 16 == 0
    trainers = [mbpe.Trainer(0) for _ in range(n_ranks)]
    for r, t in enumerate(trainers):
        t.comm_init_external(r, n_ranks)
        t.load_corpus_device(buf.data_ptr() + r * shard, shard, keep=buf)
    assert all(t.train_begin(vocab) == mbpe.NEED_EXCHANGE for t in trainers)
    _allreduce_u32(trainers)
    return trainers


def _exchange_done_codes(trainers):
    codes = []
    for t in trainers:
        try:
            codes.append(t.exchange_done())
        except mbpe.MbpeError as e:
            codes.append(e.code)
    return codes


@pytest.mark.parametrize("n_ranks", [2, 3], ids=["3GiB", "4.5GiB"])
def test_sharded_pair_sum_beyond_range_is_reported(dev, buf, n_ranks):
    """1.5 GiB of one byte per rank (every rank below 2^31 pairs on its own), the ranks' bins summed as u32: 3 Gi - 1
    pairs in all (past 2^31) and 4.5 Gi - 1 (past 2^32: the bin wraps to 0.5 Gi - 1).  Every rank reports the overflow
    from the exchange that finishes the begin -- the same decision on every rank, or a real collective would hang."""
    buf[:n_ranks * SHARD].fill_(0x60)
    torch.cuda.synchronize()
    trainers = _sharded_begin(buf, n_ranks, SHARD, 257)
    try:
        codes = _exchange_done_codes(trainers)
    finally:
        for t in trainers:
            t.close()
    assert codes == [mbpe.ERR_OVERFLOW] * n_ranks, codes


def test_sharded_top_of_int32_range_trains(dev, buf):
    """Two ranks over the 2^31-byte run of test_top_of_int32_range_trains: the same closed-form merges and counts."""
    n, k, R = 1 << 31, 31, 2
    buf[:n].fill_(ord("a"))
    torch.cuda.synchronize()
    trainers = _sharded_begin(buf, R, n // R, 256 + k)
    try:
        codes = [t.exchange_done() for t in trainers]
        assert codes == [mbpe.OK] * R
        codes = [t.train_steps(k) for t in trainers]
        while codes[0] == mbpe.NEED_EXCHANGE:
            assert codes == [mbpe.NEED_EXCHANGE] * R
            _allreduce_u32(trainers)
            codes = [t.exchange_done() for t in trainers]
        assert codes == [mbpe.OK] * R
        results = [t.train_result() for t in trainers]
    finally:
        for t in trainers:
            t.close()
    want_m, want_c = _run_merges(ord("a"), k)
    for m, c in results:
        assert m.tolist() == want_m and c.tolist() == want_c


@pytest.fixture(scope="module")
def text_corpus(dev, buf):
    """shakespeare.txt x 3,900 in buf (4.35 GB), and the oracle's pair table of one copy."""
    one = np.frombuffer(read_data("shakespeare.txt"), dtype=np.uint8)
    L = len(one)
    n = TEXT_COPIES * L
    assert n > 1 << 32
    t1 = torch.from_numpy(one.copy()).to(dev)
    buf[:n].view(TEXT_COPIES, L).copy_(t1.expand(TEXT_COPIES, L))
    del t1
    torch.cuda.synchronize()
    return one, n


def test_text_past_2_pow_32_slots_chunked(dev, buf, text_corpus):
    """Every copy its own chunk, chunk ends as slot flags: no pair crosses a copy, so the table is 3,900 x the oracle's
    of one copy, and the merges are the oracle's merges of one copy with 3,900 x its counts.  At merges 0, 10, 300 and
    1,000 the table equals a recount of the stream and the next merge is the recount's argmax."""
    one, n = text_corpus
    L = len(one)
    vocab = 256 + 1001                       # (the checkpoint at 1,000 commits merge 1,001)
    want_m, want_c = O.train(one, vocab)
    off = np.arange(TEXT_COPIES + 1, dtype=np.uint64) * np.uint64(L)
    with mbpe.Trainer(0) as tr:
        tr.set_option("chunk_barrier", 0)
        tr.load_corpus_device(buf.data_ptr(), n, off, keep=buf)
        want_t = O.pair_count_u8(one).astype(np.int64) * TEXT_COPIES
        assert np.array_equal(tr.pair_count_u8().astype(np.int64), want_t)
        tr.train_begin(vocab)
        for at in (0, 10, 300, 1000):
            have = len(tr.train_result()[0])
            if at > have:
                assert tr.train_steps(at - have) == at - have
            r = C.argmax_at_checkpoint(tr, torch, dev)
            assert r["ok"] and r["merge"] == at, r
        m, c = tr.train_result()
    assert len(m) == vocab - 256
    assert m.tolist() == want_m.tolist()
    assert c.astype(np.int64).tolist() == [TEXT_COPIES * int(x) for x in want_c]


def test_text_masked_scan_dense_cuts_around_2_pow_31_and_2_pow_32(dev, buf, text_corpus):
    """The copies of the text with further chunk ends, dense around bytes 2^31 and 2^32: at every position next to the
    boundary (inside the 16-byte vectors on either side and on their edges), at vector edges and inside vectors
    farther out.  The table is the copies' table less the pairs the new cuts take out, which are read from the device."""
    one, n = text_corpus
    L = len(one)
    rng = np.random.default_rng(31)
    cuts = set(int(x) for x in np.arange(TEXT_COPIES + 1, dtype=np.int64) * L)
    for B in (1 << 31, 1 << 32):
        cuts.update(range(B - 40, B + 41))                                   # every position around the boundary
        cuts.update(B + 16 * int(d) for d in rng.integers(-4096, 4096, size=64))            # vector edges
        cuts.update(B + 16 * int(d) + int(rng.integers(1, 16)) for d in rng.integers(-65536, 65536, size=64))   # inside
    cuts = sorted(c for c in cuts if 0 <= c <= n)
    off = np.asarray(cuts, dtype=np.uint64)
    assert off[0] == 0 and off[-1] == n
    new = torch.tensor([c for c in cuts if 0 < c < n and c % L], dtype=torch.int64, device=dev)
    a, b = buf[new - 1].long(), buf[new].long()
    taken = torch.bincount(a * 256 + b, minlength=65536).cpu().numpy().astype(np.int64)
    del new, a, b
    want = O.pair_count_u8(one).astype(np.int64) * TEXT_COPIES - taken
    with mbpe.Trainer(0) as tr:
        tr.load_corpus_device(buf.data_ptr(), n, off, keep=buf)
        got = tr.pair_count_u8().astype(np.int64)
    assert np.array_equal(got, want)
