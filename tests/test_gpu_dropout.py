"""BPE-dropout in rank order on the GPU (mbpe_encoder_set_dropout): every result is compared with the oracle of
tests/dropout_cases.py -- the numpy loop over all chunks that carries every token's byte start, which the CPU tests tie
to the literal per-chunk loop and to the stand-alone program built from csrc/dropout.h.  The shapes are laid around
groups of 64 lanes and spans of 1,024 tokens; the instance's position has to survive compaction, pieces and spans."""
import numpy as np
import pytest

import mbpe
import oracle as O
import dropout_cases as D
import encode_rank_cases as R
from conftest import read_data, read_golden
from test_gpu_encode_split import Case as DeviceCase

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

END = 0x80000000
P01 = D.threshold_of(0.1)
HALF = 1 << 31


@pytest.fixture(scope="module")
def dev():
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def _same(got, want, name):
    if len(got) != len(want) or not np.array_equal(got, want):
        n = min(len(got), len(want))
        diff = np.flatnonzero(np.asarray(got[:n]) != np.asarray(want[:n]))
        at = int(diff[0]) if len(diff) else n
        pytest.fail("%s: %d tokens, want %d; first difference at token %d: %s, want %s" % (
            name, len(got), len(want), at, got[max(at - 3, 0):at + 4].tolist(), want[max(at - 3, 0):at + 4].tolist()))


@pytest.fixture(scope="module")
def many():
    """the 5 KB many-chunk text, its table, and the oracle's result for (seed 5, p = 0.1), shared and left unchanged"""
    data, off, merges = D.many_chunk_text()
    tok, end, pos, pass_tokens = D.reference(data, off, merges, 5, P01)
    for a in (tok, end, pos):
        a.setflags(write=False)
    return data, off, merges, (tok, end, pos, pass_tokens)


@pytest.mark.parametrize("kind", ["a", "ab"])
def test_tiny_texts(kind):
    calls = 0
    with mbpe.Encoder(D.TINY_MERGES, rank_order=True) as enc:
        for n in D.TINY_LENGTHS:
            data = D.tiny_text(kind, n)
            for off in D.tiny_chunkings(n):
                for th in D.TINY_THRESHOLDS:
                    for seed in D.TINY_SEEDS:
                        enc.set_dropout(th / 2.0 ** 32, seed)       # (exact: th < 2^53)
                        tok, end, pos, pass_tokens = D.reference(data, off, D.TINY_MERGES, seed, th)
                        got, got_off = enc.encode(data, off, offsets=True)
                        name = "%s x %d, chunks %s, threshold %d, seed %d" % (kind, n, None if off is None else off.tolist(),
                                                                               th, seed)
                        _same(got, tok, name)
                        assert np.array_equal(got_off, R.chunk_tok_off(end, n, off)), name
                        if n:
                            assert enc.n_passes == len(pass_tokens) and enc.pass_tokens() == pass_tokens, name
                        if th == D.ONE:
                            assert got.tolist() == list(data), name
                        calls += 1
    assert calls == (11 + 6 + 3) * 3 * 2          # 11 lengths whole, 6 of them cut around 64, 3 around 1,024


@pytest.mark.parametrize("which", ["chain", "doubling"])
def test_nested_merges_cross_span_edges(which):
    chain = which == "chain"
    data, merges = (D.nested_chunk(), D.NESTED_MERGES) if chain else (D.doubling_chunk(), D.DOUBLING_MERGES)
    assert len(data) == 4096 and len(merges) == 10 and R.well_formed(merges)
    with mbpe.Encoder(merges, rank_order=True) as enc, mbpe.Decoder(merges) as dec:
        for th, seed in ((0, 0), (P01, 1), (P01, 2), (HALF, 1), (HALF, 99), (3 << 30, 4)):
            enc.set_dropout(th / 2.0 ** 32, seed)       # (exact: th < 2^53)
            tok, end, pos, pass_tokens = D.reference(data, None, merges, seed, th)
            print(which, th, seed, "passes", len(pass_tokens), "tokens", len(tok))
            if th == 0:
                assert len(pass_tokens) == 11                          # one pass per level and the one that ends it
                assert tok.tolist() == (([265] * 372 + [258]) if chain else [265] * 4)
            if chain and th == P01:
                assert len(pass_tokens) == 11 and len(tok) < 2048      # every level still occurs; four spans become two
            got = enc.encode(data)
            _same(got, tok, "%s, threshold %d seed %d" % (which, th, seed))
            assert enc.n_passes == len(pass_tokens) and enc.pass_tokens() == pass_tokens
            got2, boff = enc.encode(data, byte_off=True)
            _same(got2, tok, "%s with byte offsets" % which)
            assert np.array_equal(boff, D.byte_offsets(pos, len(data))), (th, seed)
            assert dec.decode(got) == data


def test_pieces_equal_the_unsplit_call(many):
    data, off, merges, (tok, end, pos, pass_tokens) = many
    assert len(data) == 5000 and len(off) > 100
    want_off = R.chunk_tok_off(end, len(data), off)
    with mbpe.Encoder(merges, rank_order=True, dropout=0.1, seed=5) as enc:
        whole, whole_off = enc.encode(data, off, offsets=True)
        _same(whole, tok, "one piece")
        assert enc.pass_tokens() == pass_tokens and np.array_equal(whole_off, want_off)
        enc.set_option("piece_bytes", 1500)
        got, got_off = enc.encode(data, off, offsets=True)
        _same(got, tok, "pieces of 1,500 bytes")                      # (the piece's base has to enter pos)
        assert np.array_equal(got_off, want_off)
        got, got_off, boff = enc.encode(data, off, offsets=True, byte_off=True)
        _same(got, tok, "pieces of 1,500 bytes with byte offsets")
        assert np.array_equal(boff, D.byte_offsets(pos, len(data)))
        # without the base every piece would draw as if it began at byte 0: the oracle says that differs
        shifted = D.dropout_loop_text(*D.token_stream(data[1500:], None)[:2], np.arange(len(data) - 1500, dtype=np.uint64),
                                      merges, 5, P01)[0]
        assert not np.array_equal(shifted, D.dropout_loop_text(*D.token_stream(data[1500:], None)[:2],
                                                               1500 + np.arange(len(data) - 1500, dtype=np.uint64),
                                                               merges, 5, P01)[0])


def test_more_than_1024_spans():
    pattern, _, merges = O.parse_model(read_golden("shakespeare_gpt4_lexical_512.model"))
    n = 1024 * 1024 + 2048 + 17
    sh = read_data("shakespeare.txt")
    data = (sh * (n // len(sh) + 1))[:n]
    off = mbpe.presplit(pattern, np.frombuffer(data, dtype=np.uint8))
    tok, end, pos, pass_tokens = D.reference(data, off, merges, 3, P01)
    assert -(-n // 1024) > 1024
    with mbpe.Encoder(merges, rank_order=True, dropout=0.1, seed=3) as enc, mbpe.Decoder(merges) as dec:
        got, got_off = enc.encode(data, off, offsets=True)
        _same(got, tok, "shakespeare x %d bytes, p = 0.1" % n)
        assert enc.pass_tokens() == pass_tokens
        assert np.array_equal(got_off, R.chunk_tok_off(end, n, off))
        assert dec.decode(got) == data
        plain = R.rank_loop_text(*R.token_stream(data, off), merges)[0]
        assert len(got) > len(plain)


def test_device_text_and_16_bit_output(dev, many):
    data, off, merges, (tok, end, pos, _) = many
    with mbpe.Encoder(merges, rank_order=True, dropout=0.1, seed=5) as enc:
        assert np.array_equal(enc.encode(data, off, dtype=np.uint16), tok.astype(np.uint16))
        text = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to(dev)
        out = torch.zeros(len(data), dtype=torch.int32, device=dev)
        boff = torch.zeros(len(data) + 1, dtype=torch.int64, device=dev)
        n, off_dev = enc.encode_device(text.data_ptr(), len(data), off, out.data_ptr(), out.numel(), offsets=True,
                                       byte_off_ptr=boff.data_ptr())
        raw = out.cpu().numpy().view(np.uint32)
        assert n == len(tok) and np.array_equal(raw[:n] & np.uint32(END - 1), tok) and not raw[n:].any()
        assert np.array_equal((raw[:n] & np.uint32(END)) != 0, end)
        assert np.array_equal(off_dev, R.chunk_tok_off(end, len(data), off))
        assert np.array_equal(boff.cpu().numpy()[:n + 1].view(np.uint64), D.byte_offsets(pos, len(data)))
        out16 = torch.zeros(len(data), dtype=torch.int16, device=dev)
        assert enc.encode_device(text.data_ptr(), len(data), off, out16.data_ptr(), out16.numel(), token_bits=16) == n
        assert np.array_equal(out16.cpu().numpy().view(np.uint16)[:n], tok.astype(np.uint16))


def test_endmask_with_singles(dev):
    s = R.special_case(as_singles=True)
    d = DeviceCase(dev, s.data, s.chunk_off, np.arange(len(s.chunk_off)))
    with mbpe.Encoder(s.merges, rank_order=True) as enc:
        for th, seed in ((P01, 2), (HALF, 8)):
            enc.set_dropout(th / 2.0 ** 32, seed)       # (exact: th < 2^53)
            tok, end, pos, _ = D.reference(s.data, s.chunk_off, s.merges, seed, th, singles=s.singles)
            assert sum(int(t) in R.SPECIAL_IDS for t in tok) == 11
            got, doc_tok = enc.encode_endmask(*d.ptrs(), singles=s.singles, doc_off=d.doc_off)
            _same(got, tok, s.name)
            assert np.array_equal(doc_tok, R.chunk_tok_off(end, len(s.data), s.chunk_off))
        assert not np.array_equal(tok, R.reference(s)[0])


def test_batch_calls(many):
    data, off, merges, (tok, end, pos, _) = many
    chunk_tok = R.chunk_tok_off(end, len(data), off)
    n_chunks = len(off) - 1
    rng = np.random.default_rng(9)
    docs = np.unique(np.concatenate([[0, n_chunks], rng.integers(0, n_chunks, size=12)])).astype(np.uint64)
    doc_tok = chunk_tok[docs.astype(np.int64)]
    with mbpe.Encoder(merges, rank_order=True, dropout=0.1, seed=5) as enc:
        for layout in ("padded", "packed"):
            kw = dict(seq_len=61, layout=layout, pad_id=3000, bos_id=None if layout == "packed" else 3001, eos_id=3002)
            want_ids, want_len = mbpe.pack_tokens(tok, doc_tok, **kw)
            ids, lengths = enc.encode_batch(data, off, docs, **kw)
            assert np.array_equal(ids, want_ids) and np.array_equal(lengths, want_len), layout
            got = enc.encode_batch_aux(data, off, docs, labels=True, positions=True, segments=True, **kw)
            want = mbpe.pack_tokens_aux(tok, doc_tok, labels=True, positions=True, segments=True, **kw)
            assert np.array_equal(enc.doc_tok_off, doc_tok), layout
            assert sorted(got) == sorted(want)
            for k in want:
                assert np.array_equal(got[k], want[k]), (layout, k)


def test_repeatable_and_seeded(many):
    data, off, merges, (tok, _, _, _) = many
    other = D.reference(data, off, merges, 6, P01)[0]
    plain = R.rank_loop_text(*R.token_stream(data, off), merges)[0]
    assert not np.array_equal(other, tok) and not np.array_equal(plain, tok)
    with mbpe.Encoder(merges, rank_order=True, dropout=0.1, seed=5) as enc, mbpe.Decoder(merges) as dec:
        a, b = enc.encode(data, off), enc.encode(data, off)
        _same(a, tok, "seed 5")
        assert np.array_equal(a, b)                                    # the same call twice
        enc.set_dropout(0.1, 6)
        _same(enc.encode(data, off), other, "seed 6")                  # differs wherever the oracle says it does
        enc.set_dropout(0.0)
        _same(enc.encode(data, off), plain, "set_dropout(0) after p > 0")
        for p in (0.0, 0.1, 0.5, 0.9, 1.0):
            enc.set_dropout(p, 77)
            got = enc.encode(data, off)
            _same(got, D.reference(data, off, merges, 77, D.threshold_of(p))[0], "p = %g" % p)
            assert dec.decode(got) == data
            if p == 1.0:
                assert got.tolist() == list(data)


def test_threshold_zero_allocates_and_launches_as_before(many):
    data, off, merges, _ = many

    def calls(enc):
        enc.encode(data, off)
        enc.encode(data, off, byte_off=True)
        enc.encode_batch(data, off, None, seq_len=32)
        return enc.alloc_count()
    with mbpe.Encoder(merges, rank_order=True) as never, mbpe.Encoder(merges, rank_order=True) as zero, \
            mbpe.Encoder(merges, rank_order=True) as on:
        zero.set_dropout(0.0, 123)
        on.set_dropout(0.1, 123)
        a_never, a_zero, a_on = calls(never), calls(zero), calls(on)
        assert a_zero == a_never
        assert a_on == a_never + 2                                     # the two arrays of byte starts
        assert calls(on) == a_on                                       # and a repeat allocates nothing
        on.set_dropout(0.0)
        assert np.array_equal(on.encode(data, off), never.encode(data, off))
        assert never.pass_tokens() == on.pass_tokens()


def test_error_cases(many):
    data, off, merges, (tok, _, _, _) = many
    with mbpe.Encoder(merges) as enc:
        with pytest.raises(mbpe.MbpeError) as e:
            mbpe._check(mbpe.lib().mbpe_encoder_set_dropout(enc._h, (1 << 32) + 1, 0))
        assert e.value.code == mbpe.ERR_ARG
        mbpe._check(mbpe.lib().mbpe_encoder_set_dropout(enc._h, 1 << 32, 0))
        enc.set_dropout(0.0)
        for bad in (-0.5, 1.5, float("nan")):
            with pytest.raises(mbpe.MbpeError) as e:
                enc.set_dropout(bad)
            assert e.value.code == mbpe.ERR_ARG
        greedy = enc.encode(data, off)
        enc.set_dropout(0.1, 5)                                        # p > 0 with rank_order 0: every encode call refuses
        for call in (lambda: enc.encode(data, off), lambda: enc.encode(data, off, byte_off=True),
                     lambda: enc.encode_batch(data, off, None, seq_len=32),
                     lambda: enc.encode_batch_aux(data, off, None, seq_len=32, labels=True)):
            with pytest.raises(mbpe.MbpeError) as e:
                call()
            assert e.value.code == mbpe.ERR_ARG and "rank_order" in str(e.value)
        enc.set_option("rank_order", 1)                                # the encoder stays usable, in either way out
        _same(enc.encode(data, off), tok, "after the refusal")
        enc.set_option("rank_order", 0)
        enc.set_dropout(0.0)
        assert np.array_equal(enc.encode(data, off), greedy)
