"""mbpe_encoder_count and mbpe_encoder_count_endmask: the token frequency table of a text, counted on the device without
a token leaving it, on every route an encode call can take.  The reference is np.bincount of what the SAME encoder's
encode call returns for the same arguments (its own tests hold that to the Python loops); equality is exact."""
import numpy as np
import pytest

import mbpe
import oracle as O
import dedup_cases as D
import expand_cases as X
import hist_cases as H
from conftest import read_data, read_golden

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ORDERS = ("greedy", "rank")
REAL = O.parse_model(read_golden("taylorswift_gpt4_lexical_512.model"))[2]
SPECIALS = {b"<|endoftext|>": 100257, b"<|fim_prefix|>": 600}


@pytest.fixture(scope="module")
def dev():
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def swift():
    """The first 64 KiB of taylorswift.txt with its gpt4 chunks."""
    data = np.frombuffer(read_data("taylorswift.txt")[:65536], dtype=np.uint8)
    return data, mbpe.presplit(O.GPT4_SPLIT_PATTERN, data)


def table_of(enc, tokens, weight=1):
    """What counts() must return after `tokens` were counted `weight` times into an empty table."""
    n_ids = len(enc.counts()[0])
    want, other = H.reference(tokens, n_ids)
    return want * np.uint64(weight), other * weight, len(tokens) * weight


def assert_table(enc, want):
    counts, other, total = enc.counts()
    assert counts.dtype == np.uint64 and np.array_equal(counts, want[0]) and (other, total) == (want[1], want[2])
    assert int(counts.sum()) + other == total


def count_equals_encode(enc, data, off, text_dev=None):
    """count() into an empty table against the bincount of encode(); with text_dev the device text as well."""
    tokens = enc.encode(data, off)
    enc.reset_counts()
    assert enc.count(data, off) == len(tokens)
    assert_table(enc, table_of(enc, tokens))
    if text_dev is not None:
        enc.reset_counts()
        assert enc.count_device(text_dev.data_ptr(), len(data), off) == len(tokens)
        assert_table(enc, table_of(enc, tokens))
    return tokens


@pytest.mark.parametrize("dedup", [False, True])
@pytest.mark.parametrize("order", ORDERS)
def test_routes(dev, swift, order, dedup):
    data, off = swift
    text = torch.from_numpy(np.concatenate([data, np.zeros(16, dtype=np.uint8)])).to(dev)
    with mbpe.Encoder(REAL, rank_order=order == "rank", dedup=dedup) as enc:
        assert len(enc.counts()[0]) == 256 + len(REAL) and enc.counts()[1:] == (0, 0)       # before the first count: zeros
        tokens = count_equals_encode(enc, data, off, text)
        assert 0 < len(tokens) < len(data) and enc.kernel_ms() > 0
        # a repeat call allocates nothing; two calls are the count of the concatenation; repeat 3
        before = enc.alloc_count()
        assert enc.count(data, off) == len(tokens)
        assert enc.alloc_count() == before
        assert_table(enc, table_of(enc, tokens, 2))
        half = int(np.searchsorted(off, 30000))
        enc.reset_counts()
        enc.count(data[:int(off[half])], off[:half + 1])
        enc.count(data[int(off[half]):], off[half:] - off[half], repeat=1)
        assert_table(enc, table_of(enc, tokens))
        assert enc.alloc_count() == before
        enc.reset_counts()
        assert_table(enc, table_of(enc, tokens[:0]))
        enc.count(data, off, repeat=3)
        assert_table(enc, table_of(enc, tokens, 3))
        # at least three pieces (the "dedup" route runs the unique text as one piece: 24,000 bytes hold it)
        enc.set_option("piece_bytes", 24000)
        count_equals_encode(enc, data, off, text)
        # one chunk, and no text at all
        enc.set_option("piece_bytes", 0)
        count_equals_encode(enc, data[:5000], None)
        enc.reset_counts()
        assert enc.count(b"") == 0 and enc.count(data[:0], np.zeros(4, dtype=np.uint64)) == 0
        assert_table(enc, table_of(enc, tokens[:0]))


def test_dropout_on_the_plain_route(dev, swift):
    data, off = swift
    with mbpe.Encoder(REAL, rank_order=True, dropout=0.3, seed=11) as enc, mbpe.Encoder(REAL, rank_order=True) as plain:
        tokens = count_equals_encode(enc, data, off)
        assert len(tokens) > len(plain.encode(data, off))          # the dropout is at work
        enc.set_option("piece_bytes", 24000)
        count_equals_encode(enc, data, off)
        # with "dedup" it stays an argument error, and the table stays
        enc.set_option("dedup", 1)
        before = enc.counts()
        with pytest.raises(mbpe.MbpeError) as e:
            enc.count(data, off)
        assert e.value.code == mbpe.ERR_ARG
        after = enc.counts()
        assert np.array_equal(before[0], after[0]) and before[1:] == after[1:]


@pytest.mark.parametrize("dedup", [False, True])
def test_empty_chunks(dev, dedup):
    chunks = X.edge_chunks(1500, seed=3)
    data, off = X.with_empty_chunks(chunks)
    text = torch.from_numpy(np.concatenate([data, np.zeros(16, dtype=np.uint8)])).to(dev)
    with mbpe.Encoder(REAL, dedup=dedup) as enc:
        count_equals_encode(enc, data, off, text)


@pytest.mark.parametrize("dedup", [False, True])
@pytest.mark.parametrize("count_ids", [None, 70000])
def test_nul_led_chunks(dev, dedup, count_ids):
    # one-token chunks with the ids 300, 77 and 65,000: inside the table with count_ids, beyond it (n_other) without
    data, off = D.join(X.nul_chunks())
    text = torch.from_numpy(np.concatenate([data, np.zeros(16, dtype=np.uint8)])).to(dev)
    with mbpe.Encoder(X.NEVER, dedup=dedup, count_ids=count_ids) as enc:
        tokens = count_equals_encode(enc, data, off, text)
        counts, other, total = enc.counts()
        assert len(counts) == (257 if count_ids is None else 70000) and counts[77] == 5
        if count_ids is None:
            assert other == 15                                    # 300 twice and 65,000 once, five times over
        else:
            assert other == 0 and counts[300] == 10 and counts[65000] == 5
        assert total == len(tokens)


@pytest.mark.parametrize("dedup", [False, True])
@pytest.mark.parametrize("order", ORDERS)
def test_endmask_route_with_singles(dev, order, dedup):
    docs = [read_data("taylorswift.txt")[:20000], b"<|endoftext|>", b"", b"a<|fim_prefix|>b<|endoftext|><|endoftext|> the end",
            read_data("specialtokensample.txt")]
    data = np.frombuffer(b"".join(docs), dtype=np.uint8)
    doc_off = np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.uint64)
    names = sorted(SPECIALS)
    with mbpe.Splitter(O.GPT4_SPLIT_PATTERN) as sp, mbpe.Encoder(REAL, rank_order=order == "rank", dedup=dedup) as enc:
        n_chunks, ranges = sp.split_docs(data, doc_off, names=names)
        singles = [(int(s), int(n), SPECIALS[names[int(k)]]) for s, n, k in ranges if k != mbpe.SPLIT_RAW]
        assert len(singles) >= 4 and n_chunks > 1000
        mask_ptr, _, text_ptr = sp.endmask()
        tokens, _ = enc.encode_endmask(text_ptr, len(data), mask_ptr, singles=singles)
        assert (tokens == 100257).sum() >= 3 and (tokens == 600).sum() >= 1
        enc.reset_counts()
        assert enc.count_endmask(text_ptr, len(data), mask_ptr, singles=singles) == len(tokens)
        assert_table(enc, table_of(enc, tokens))
        assert enc.counts()[1] >= 3                               # 100,257 and 600 lie beyond the 512 bins
        before = enc.alloc_count()
        assert enc.count_endmask(text_ptr, len(data), mask_ptr, singles=singles, repeat=4) == len(tokens)
        assert_table(enc, table_of(enc, tokens, 5))
        assert enc.alloc_count() == before
        # the table on the device
        out = torch.full((len(enc.counts()[0]) + 1,), -1, dtype=torch.int64, device=dev)
        n_ids, other, total = enc.counts(out_ptr=out.data_ptr())
        raw = out.cpu().numpy()
        assert n_ids == 256 + len(REAL) and np.array_equal(raw[:n_ids].view(np.uint64), enc.counts()[0]) and raw[n_ids] == -1


DEDUP_SHAPES = {"distinct-600": X.distinct_chunks(), "equal-600": X.equal_chunks(600), "residue-0": X.residue_chunks(0),
                "residue-5": X.residue_chunks(5), "residue-7": X.residue_chunks(7), "long": X.long_chunks()}


@pytest.mark.parametrize("table", ["never", "real"])
@pytest.mark.parametrize("name", sorted(DEDUP_SHAPES))
def test_dedup_shapes(dev, name, table):
    chunks = DEDUP_SHAPES[name]
    data, off = D.join(chunks)
    with mbpe.Encoder(X.NEVER if table == "never" else REAL, dedup=True) as enc:
        count_equals_encode(enc, data, off)
        st = enc.dedup_stats()
        assert st["n_chunks"] == len(chunks) and st["n_unique"] == len(D.dedup(chunks)[0])


@pytest.mark.parametrize("max_chunk", [None, 0])
def test_dedup_long_chunk_and_no_hashing(dev, max_chunk):
    # a 300,000-byte chunk, far above max_chunk_bytes, twice between words: it passes the deduper unhashed, and its run
    # of up to 300,000 tokens is counted element by element.  "dedup_max_chunk_bytes" 0: nothing is hashed at all
    rng = np.random.default_rng(5)
    big = bytes(rng.integers(97, 123, size=300000, dtype=np.uint8))
    chunks = [b" the", big, b" the", b" end", big, b" the"]
    data, off = D.join(chunks)
    for merges in (X.NEVER, REAL):
        with mbpe.Encoder(merges, dedup=True) as enc:
            if max_chunk is not None:
                enc.set_option("dedup_max_chunk_bytes", max_chunk)
            count_equals_encode(enc, data, off)
            assert enc.dedup_stats()["n_unique"] == (4 if max_chunk is None else 6)


@pytest.mark.parametrize("dedup", [False, True])
def test_repeat_at_the_64_bit_limits(dev, dedup):
    with mbpe.Encoder(X.NEVER, dedup=dedup) as enc:
        tokens = enc.encode(b"aaab")
        assert tokens.tolist() == [97, 97, 97, 98]
        assert enc.count(b"aaab", repeat=1 << 61) == 4            # the count itself carries no repeat
        counts, other, total = enc.counts()
        assert int(counts[97]) == 3 << 61 and int(counts[98]) == 1 << 61 and other == 0 and total == 1 << 63
        assert sum(int(c) for c in counts) == 1 << 63
        # 4 * 2^62 = 2^64, and so is 2^63 + 4 * 2^61: refused on the host, the table unchanged
        for rep in (1 << 62, 1 << 61):
            with pytest.raises(mbpe.MbpeError) as e:
                enc.count(b"aaab", repeat=rep)
            assert e.value.code == mbpe.ERR_OVERFLOW
            again = enc.counts()
            assert np.array_equal(again[0], counts) and again[1:] == (other, total)
        assert enc.count(b"aaab", repeat=(1 << 61) - 1) == 4      # 2^64 - 4 is reached exactly
        counts, other, total = enc.counts()
        assert int(counts[97]) == (3 << 62) - 3 and int(counts[98]) == (1 << 62) - 1 and total == (1 << 64) - 4
        with pytest.raises(mbpe.MbpeError) as e:
            enc.count(b"aaab", repeat=0)
        assert e.value.code == mbpe.ERR_ARG
        enc.reset_counts()
        enc.count(b"aaab", repeat=1 << 61)
        assert enc.counts()[2] == 1 << 63


def test_errors_leave_the_table_unchanged(dev, swift):
    data, off = swift
    with mbpe.Encoder(REAL) as enc:
        tokens = enc.encode(data[:20000], off[:np.searchsorted(off, 20000)].tolist() + [20000])
        enc.count(data[:20000], off[:np.searchsorted(off, 20000)].tolist() + [20000])
        want = table_of(enc, tokens)
        assert_table(enc, want)
        # a chunk longer than a piece: MBPE_ERR_OOM, although the pieces before it fit
        enc.set_option("piece_bytes", 4000)
        long_off = np.concatenate([off[off < 30000], [40000], off[off > 40000]]).astype(np.uint64)
        with pytest.raises(mbpe.MbpeError) as e:
            enc.count(data, long_off)
        assert e.value.code == mbpe.ERR_OOM
        assert_table(enc, want)
        # chunk offsets that do not end at n_bytes
        with pytest.raises(mbpe.MbpeError) as e:
            enc.count(data, off[:-1])
        assert e.value.code == mbpe.ERR_ARG
        assert_table(enc, want)
        # "count_ids" once something has been counted; after a reset it may change, and the table follows
        for value in (0, 5000):
            with pytest.raises(mbpe.MbpeError) as e:
                enc.set_option("count_ids", value)
            assert e.value.code == mbpe.ERR_STATE
        for value in (-1, (1 << 25) + 1):
            with pytest.raises(mbpe.MbpeError) as e:
                enc.set_option("count_ids", value)
            assert e.value.code == mbpe.ERR_ARG
        assert_table(enc, want)
        enc.reset_counts()
        enc.set_option("count_ids", 5000)
        enc.set_option("piece_bytes", 0)
        enc.count(data[:20000], off[:np.searchsorted(off, 20000)].tolist() + [20000])
        assert len(enc.counts()[0]) == 5000
        assert_table(enc, table_of(enc, tokens))
        enc.reset_counts()
        enc.set_option("count_ids", 0)
        assert len(enc.counts()[0]) == 256 + len(REAL)
        enc.count(data[:20000], off[:np.searchsorted(off, 20000)].tolist() + [20000])
        assert_table(enc, table_of(enc, tokens))


def test_an_encoder_that_never_counts_allocates_what_it_did(dev, swift):
    # the buffers of a plain encode call: the same number with and without a count call between two of them, less the
    # two tables the count call brought
    data, off = swift
    with mbpe.Encoder(REAL) as a, mbpe.Encoder(REAL) as b:
        a.encode(data, off)
        b.encode(data, off)
        base = a.alloc_count()
        assert b.alloc_count() == base
        b.count(data, off)
        assert b.alloc_count() == base + 2                        # the kept table and the call's scratch
        a.encode(data, off)
        b.encode(data, off)
        assert a.alloc_count() == base and b.alloc_count() == base + 2
