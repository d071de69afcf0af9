"""The device planner of the fit layout (csrc/pack_fit_dev.hip) against the reference planner fit_cases.ref_plan:
mbpe.pack_fit_plan(..., device=0) gives its n_rows, lengths, doc_row and doc_col exactly; Encoder(fit_planner="device")
and Tokenizer.set_fit_planner("device") give the matrices of the host planner, and fit_stats says who planned."""
import random

import numpy as np
import pytest

import mbpe
import oracle as O
from conftest import read_golden
from fit_cases import grid_lengths, plan_outputs, ref_plan

pytestmark = pytest.mark.gpu

BOS_EOS = [(None, None), (5, None), (None, 6), (5, 6)]
ALL = dict(labels=True, positions=True, segments=True, doc_row=True, doc_col=True)


def check_plan(lens, S, bos=None, eos=None):
    nbe = (bos is not None) + (eos is not None)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    placed, n_rows = ref_plan([n + nbe for n in lens], S)
    length, doc_row, doc_col = plan_outputs(placed, n_rows, len(lens))
    got = mbpe.pack_fit_plan(off, S, bos, eos, device=0)
    assert got["n_rows"] == n_rows
    assert got["lengths"].tolist() == length
    assert got["doc_row"].tolist() == doc_row and got["doc_col"].tolist() == doc_col


@pytest.mark.parametrize("S", [1, 2, 3, 5, 8, 13, 16, 64])
@pytest.mark.parametrize("bos,eos", BOS_EOS)
def test_grid_equals_the_reference(S, bos, eos):
    check_plan(grid_lengths(S, (bos is not None) + (eos is not None)), S, bos, eos)


@pytest.mark.parametrize("S", [16, 64])
@pytest.mark.parametrize("n_docs", [200, 2000])
def test_random_lists_equal_the_reference(S, n_docs):
    """Lengths in [0, 2 S + 1]: scrambled buckets, a row left with room when its class runs out, buckets consumed in part."""
    rng = random.Random(1000 * S + n_docs)
    check_plan([rng.randrange(0, 2 * S + 2) for _ in range(n_docs)], S)
    check_plan([rng.randrange(0, 2 * S + 2) for _ in range(n_docs)], S, 5, 6)


def test_a_bucket_beyond_the_lds_sort():
    """70,000 tails of 33 open as many rows with room 31, appended in any order; the 150 tails of 31 take the lowest 150:
    the bucket is sorted through global memory.  No documents: an empty plan."""
    lens = [33] * 70000 + [31] * 150
    random.Random(7).shuffle(lens)
    check_plan(lens, 64)
    check_plan([], 64)


def byte_texts(lens, rng):
    return [bytes(rng.randrange(97, 123) for _ in range(n)) for n in lens]


@pytest.mark.parametrize("S,planner", [(16, 1), (64, 1), (mbpe.FIT_DEVICE_MAX_SEQ, 1), (mbpe.FIT_DEVICE_MAX_SEQ + 1, 0)])
def test_encoder_option_equals_the_host_planner(S, planner):
    """No merges: a document's tokens are its bytes.  At the bound the device plans, one above it the host does."""
    rng = random.Random(S)
    n_docs = 300 if S <= 64 else 12
    texts = byte_texts([rng.randrange(0, 2 * S + 2) for _ in range(n_docs)], rng)
    kw = dict(seq_len=S, pad_id=0, bos_id=1, eos_id=2, **ALL)
    none = np.zeros((0, 2), dtype=np.uint32)
    with mbpe.Encoder(none) as host, mbpe.Encoder(none, fit_planner="device") as enc:
        assert enc.fit_stats() == (0, 0, 0, 0)
        want = host.encode_batch_fit(texts, **kw)
        got = enc.encode_batch_fit(texts, **kw)
        assert host.fit_stats()[0] == 0 and enc.fit_stats()[0] == planner
        assert enc.fit_stats()[1:3] == host.fit_stats()[1:3] and enc.fit_stats()[1] > 0
        assert sorted(got) == sorted(want)
        for k in want:
            assert np.array_equal(got[k], want[k]), k
        allocs = enc.alloc_count()
        again = enc.encode_batch_fit(texts[:-1], **kw)             # a repeat call of no larger size
        assert enc.alloc_count() == allocs
        assert np.array_equal(again["doc_row"], host.encode_batch_fit(texts[:-1], **kw)["doc_row"])
        enc.set_option("fit_planner", 0)
        enc.encode_batch_fit(texts, **kw)
        assert enc.fit_stats()[0] == 0


def test_tokenizer_setter_equals_the_host_planner():
    pattern, _, merges = O.parse_model(read_golden("taylorswift_gpt4_first_512.model"))
    texts = [b"Hello world, hello there.", b"", b"a", b"The quick brown fox jumps over the lazy dog. " * 3, b"bcd efg"] * 5
    kw = dict(seq_len=16, eos_id=100257, **ALL)
    t = mbpe.Tokenizer(pattern)
    try:
        t.set_merges(merges)
        want = t.encode_batch_fit(texts, **kw)
        t.set_fit_planner("device")
        got = t.encode_batch_fit(texts, **kw)
        t.set_fit_planner("host")
        assert sorted(got) == sorted(want)
        for k in want:
            assert np.array_equal(got[k], want[k]), k
    finally:
        t.close()
