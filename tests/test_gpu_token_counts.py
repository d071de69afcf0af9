"""mbpe_token_counts (csrc/hist.hip): the histogram of ids that exist already, against np.bincount of the generated ids
-- exact.  The shapes (tests/hist_cases.py) lie around a lane's piece of 16 bytes, a span of 1,024 and a workgroup's tile
of 4,096 positions, around every power of two an id can straddle kHistLocalIds at, and at table sizes from 1 to
MBPE_MAX_COUNT_IDS."""
import numpy as np
import pytest

import mbpe
import hist_cases as H

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def dev():
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def check(tokens, n_ids, ids=None):
    """Host tokens, host table -> must be the bincount of ids (default: the tokens themselves)."""
    want, want_other = H.reference(tokens if ids is None else ids, n_ids)
    got, other = mbpe.token_counts(tokens, n_ids)
    assert got.dtype == np.uint64 and len(got) == n_ids
    assert other == want_other and np.array_equal(got, want)
    assert int(got.sum()) + other == len(tokens)


@pytest.mark.parametrize("n", H.LENGTHS)
def test_lengths(dev, n):
    tokens = H.edge_tokens(n)
    for n_ids in (257, 65537):
        check(tokens, n_ids)
    # device tokens at every element offset within 16 bytes (the head and the tail of the aligned pieces)
    want, want_other = H.reference(tokens, 65537)
    for shift in (0, 1, 2, 3):
        host = np.concatenate([np.full(shift, 5, dtype=np.uint32), tokens, np.full(4, 7, dtype=np.uint32)])
        buf = torch.from_numpy(host.view(np.int32)).to(dev)
        got, other = mbpe.token_counts(None, 65537, tokens_ptr=buf.data_ptr() + 4 * shift, n_tokens=n, token_bits=32)
        assert other == want_other and np.array_equal(got, want), shift


@pytest.mark.parametrize("n_ids", H.N_IDS)
def test_table_sizes(dev, n_ids):
    check(H.edge_tokens(4097), n_ids)
    check(H.edge_tokens(0), n_ids)                      # no token: zeros


@pytest.mark.parametrize("n_ids", [257, 65537])
def test_all_tokens_equal(dev, n_ids):
    # (n_ids - 1 = 65,536 lies beyond every kHistLocalIds: the direct global atomics; 256 lies below it: one LDS address)
    for value in (0, n_ids - 1, n_ids, 0x7FFFFFFF):
        tokens = np.full(20000, value, dtype=np.uint32)
        got, other = mbpe.token_counts(tokens, n_ids)
        if value < n_ids:
            assert other == 0 and got[value] == 20000 and int(got.sum()) == 20000
        else:
            assert other == 20000 and not got.any()


@pytest.mark.parametrize("draw", ["zipf", "uniform"])
def test_draws_over_2_24_ids(dev, draw):
    n = (1 << 20) + 3
    tokens = H.zipf_tokens(n, 1 << 24) if draw == "zipf" else H.uniform_tokens(n, 1 << 24)
    check(tokens, 1 << 24)
    check(tokens, 5000)                                 # most of a uniform draw goes to `other`


def test_16_bit_ids_with_65535(dev):
    for n in (1, 7, 8, 9, 4097, 70001):
        t = H.edge_tokens(n).astype(np.uint16)
        t[::5] = 65535
        for n_ids in (65536, 65535, 257):
            check(t, n_ids)
        want, want_other = H.reference(t, 65536)
        for shift in (1, 5, 7):
            host = np.concatenate([np.full(shift, 5, dtype=np.uint16), t, np.full(8, 7, dtype=np.uint16)])
            buf = torch.from_numpy(host.view(np.int16)).to(dev)
            got, other = mbpe.token_counts(None, 65536, tokens_ptr=buf.data_ptr() + 2 * shift, n_tokens=n, token_bits=16)
            assert other == want_other and np.array_equal(got, want), shift


def test_bit_31_is_cleared(dev):
    ids = H.edge_tokens(70001)
    tokens = H.flagged(ids, every=3)
    assert (tokens[::3] >> 31).all()
    for n_ids in (257, 65537, 1 << 24):
        check(tokens, n_ids, ids=ids)


@pytest.mark.parametrize("tokens_on_device", [False, True])
@pytest.mark.parametrize("out_on_device", [False, True])
def test_host_and_device_sides(dev, tokens_on_device, out_on_device):
    tokens, n_ids = H.edge_tokens(70001), 65537
    want, want_other = H.reference(tokens, n_ids)
    d_tok = torch.from_numpy(tokens.view(np.int32).copy()).to(dev)
    src = dict(tokens_ptr=d_tok.data_ptr(), n_tokens=len(tokens), token_bits=32) if tokens_on_device else {}
    if out_on_device:
        out = torch.full((n_ids + 2,), 0x5A5A5A5A, dtype=torch.int64, device=dev)       # WRITES: what was there is gone
        other = mbpe.token_counts(None if tokens_on_device else tokens, n_ids, out_ptr=out.data_ptr(), **src)
        raw = out.cpu().numpy().view(np.uint64)
        got = raw[:n_ids]
        assert (raw[n_ids:] == 0x5A5A5A5A).all()
    else:
        got, other = mbpe.token_counts(None if tokens_on_device else tokens, n_ids, **src)
    assert other == want_other and np.array_equal(got, want)
    assert mbpe.token_counts_kernel_ms() > 0


def test_argument_errors(dev):
    tokens = H.edge_tokens(100)
    d_tok = torch.from_numpy(np.zeros(64, dtype=np.int32)).to(dev)
    for n_ids in (0, (1 << 25) + 1):
        with pytest.raises(mbpe.MbpeError) as e:
            mbpe.token_counts(tokens, n_ids)
        assert e.value.code == mbpe.ERR_ARG
    for shift, bits in ((1, 32), (2, 32), (1, 16)):
        with pytest.raises(mbpe.MbpeError) as e:
            mbpe.token_counts(None, 300, tokens_ptr=d_tok.data_ptr() + shift, n_tokens=8, token_bits=bits)
        assert e.value.code == mbpe.ERR_ARG
    with pytest.raises(mbpe.MbpeError) as e:
        mbpe.token_counts(None, 300, tokens_ptr=d_tok.data_ptr(), n_tokens=8, token_bits=8)
    assert e.value.code == mbpe.ERR_ARG
    with pytest.raises(mbpe.MbpeError) as e:
        mbpe.token_counts(tokens, 300, out_ptr=d_tok.data_ptr() + 4)
    assert e.value.code == mbpe.ERR_ARG
