"""Token byte offsets at the encoder level (mbpe_encoder_encode_byteoff, mbpe_encoder_encode_endmask_byteoff) on the
GPU, against the position-carrying BPE of byteoff_cases.py: token counts at every edge of the span walk, one-token
chunks on both routes, pieces, the other call forms, tables the calls refuse, and offsets beyond 2^32."""
import ctypes

import numpy as np
import pytest

import mbpe
import oracle as O
import byteoff_cases as B
from conftest import read_data

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

SPAN = 1024
GPT4 = O.GPT4_SPLIT_PATTERN


@pytest.fixture(scope="module")
def dev():
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def random_text(seed, n, letters=b"abcd"):
    rng = np.random.default_rng(seed)
    return np.frombuffer(letters, dtype=np.uint8)[rng.integers(0, len(letters), n)].copy()


@pytest.fixture(scope="module")
def table():
    """A small trained table over four letters: token lengths of 1, 2 and 3 bytes."""
    merges, _ = O.train(random_text(1, 4096), 256 + 12)
    merges = np.ascontiguousarray(merges, dtype=np.uint32).reshape(-1, 2)
    assert len(merges) == 12
    mbpe.merges_check(merges)
    return merges


def chunked(seed, n_bytes):
    """Random letters cut into chunks of 1 .. 9 bytes."""
    rng = np.random.default_rng(seed)
    data = random_text(seed + 1000, n_bytes)
    cuts = np.unique(np.concatenate([[0, n_bytes], rng.integers(0, n_bytes + 1, max(n_bytes // 5, 1))]))
    return data, cuts.astype(np.uint64)


def with_n_tokens(table, n_tokens, rank):
    """A chunked text whose encoding has exactly n_tokens tokens: whole chunks of a random text, then one-byte chunks
    (one token each) up to the count."""
    data, off = chunked(n_tokens, 3 * n_tokens + 16)
    lookup = {tuple(m): 256 + k for k, m in enumerate(table.tolist())}
    total, k = 0, 0
    while k + 1 < len(off):
        t = len(B.encode_chunk(bytes(data[int(off[k]):int(off[k + 1])]), 0, lookup, rank))
        if total + t > n_tokens:
            break
        total += t
        k += 1
    head = int(off[k])
    pad = n_tokens - total
    text = np.concatenate([data[:head], random_text(7, pad)])
    chunk_off = np.concatenate([off[:k + 1], head + 1 + np.arange(pad, dtype=np.uint64)]).astype(np.uint64)
    return text, chunk_off


def check(got, want, name):
    (tokens, boff), (want_t, want_b) = got, want
    assert tokens.tolist() == want_t.tolist(), name
    assert boff.dtype == np.uint64 and len(boff) == len(tokens) + 1, name
    if not np.array_equal(boff, want_b):
        at = int(np.flatnonzero(boff != want_b)[0])
        pytest.fail("%s: tok_byte_off[%d] = %d, want %d" % (name, at, boff[at], want_b[at]))


@pytest.mark.parametrize("rank", [False, True], ids=["greedy", "rank"])
@pytest.mark.parametrize("n_tokens", [0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 2048, 2049])
def test_token_counts_at_every_edge_of_the_walk(dev, table, n_tokens, rank):
    text, off = with_n_tokens(table, n_tokens, rank)
    want = B.encode_chunks(text, off, table, rank)
    assert len(want[0]) == n_tokens
    with mbpe.Encoder(table, rank_order=rank) as enc:
        check(enc.encode(text, off, byte_off=True), want, "chunks")
        assert enc.encode(text, off).tolist() == want[0].tolist()
        if n_tokens:                                              # as ONE chunk: other tokens, the same contract
            check(enc.encode(text, None, byte_off=True), B.encode_chunks(text, None, table, rank), "one chunk")


def test_more_than_1024_spans(dev):
    """More than 1,048,576 final tokens: a scan thread owns two spans.  The tokens are the plain call's; the offsets
    are the running sum of the tokens' lengths, and the tokens' bytes in a row are the text."""
    rng = np.random.default_rng(11)
    text = rng.integers(0, 256, 3 << 20, dtype=np.uint8)
    merges = np.array([[97, 98], [0, 0], [256, 99], [1, 2], [257, 257], [200, 201]], dtype=np.uint32)
    vocab = B.vocab_bytes(merges.tolist())
    lens = np.array([len(v) for v in vocab], dtype=np.uint64)
    with mbpe.Encoder(merges) as enc:
        tokens, boff = enc.encode(text, None, byte_off=True)
        assert len(tokens) > 1024 * SPAN + SPAN
        assert tokens.tolist() == enc.encode(text).tolist()
    want = np.concatenate([[0], np.cumsum(lens[tokens], dtype=np.uint64)]).astype(np.uint64)
    assert np.array_equal(boff, want) and boff[-1] == len(text)
    assert b"".join(vocab[t] for t in tokens.tolist()) == text.tobytes()


# ---- one-token chunks --------------------------------------------------------------------------------------------

def marker_case(table):
    """Host-chunk route: "\\0<id>" chunks as first chunk, as last chunk, two adjacent at output indices 1,023 and 1,024,
    one whose chunk is longer than what its id decodes to, one whose id is beyond the vocabulary."""
    text, off = with_n_tokens(table, 1022, False)
    parts, cuts = [b"\x00 97"], [4]                                # index 0: 'a', a chunk of 4 bytes for a 1-byte id
    parts.append(text.tobytes())
    cuts += (off[1:].astype(np.int64) + 4).tolist()                # indices 1 .. 1,022
    for marker in (b"\x00 \t  260", b"\x00100257"):                # indices 1,023 and 1,024: adjacent, on the span edge
        parts.append(marker)
        cuts.append(cuts[-1] + len(marker))
    tail, tail_off = chunked(5, 300)
    parts.append(tail.tobytes())
    cuts += (tail_off[1:].astype(np.int64) + cuts[-1]).tolist()
    parts.append(b"\x007")
    cuts.append(cuts[-1] + 2)
    data = np.frombuffer(b"".join(parts), dtype=np.uint8)
    return data, np.array([0] + cuts, dtype=np.uint64)


@pytest.mark.parametrize("rank", [False, True], ids=["greedy", "rank"])
def test_marker_chunks_cover_their_whole_chunk(dev, table, rank):
    data, off = marker_case(table)
    want = B.encode_chunks(data, off, table, rank)
    if not rank:
        assert want[0][0] == 97 and want[0][1023] == 260 and want[0][1024] == 100257 and want[0][-1] == 7
        assert want[1][1] == 4 and want[1][1024] - want[1][1023] == 8
    with mbpe.Encoder(table, rank_order=rank) as enc:
        check(enc.encode(data, off, byte_off=True), want, "markers")
        tokens, tok_off, boff = enc.encode(data, off, offsets=True, byte_off=True)     # with the chunk offsets too
        check((tokens, boff), want, "markers + chunk offsets")
        assert boff[tok_off.astype(np.int64)].tolist() == off.tolist()                  # a chunk's tokens cover it
        enc.set_option("piece_bytes", 512)                        # markers in later pieces: their index is piece-local
        check(enc.encode(data, off, byte_off=True), want, "markers in pieces")


class MaskCase:
    """A text and its end mask on the device, with the chunk offsets read off the mask."""

    def __init__(self, dev, data, chunk_off=None, names=None):
        self.data = np.ascontiguousarray(np.frombuffer(bytes(data), dtype=np.uint8))
        n = len(self.data)
        self.d_text = torch.from_numpy(self.data.copy()).to(dev)
        self.singles = []
        if chunk_off is None:                                     # the device split, around the names
            self.d_mask = torch.zeros(mbpe.Splitter.mask_bytes(n), dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            with mbpe.Splitter(GPT4) as sp:
                _, rows = sp.split_docs(self.data, [0, n], list(names), mask_ptr=self.d_mask.data_ptr())
            ids = list(names.values())
            self.singles = [(int(s), int(l), ids[int(k)]) for s, l, k in rows.tolist()]
            bits = np.unpackbits(self.d_mask.cpu().numpy(), bitorder="little")[:n]
            self.off = np.concatenate([[0], np.flatnonzero(bits) + 1]).astype(np.uint64)
        else:
            self.off = np.ascontiguousarray(chunk_off, dtype=np.uint64)
            bits = np.zeros(mbpe.Splitter.mask_bytes(n) * 8, dtype=np.uint8)
            bits[self.off[1:].astype(np.int64) - 1] = 1
            self.d_mask = torch.from_numpy(np.packbits(bits, bitorder="little")).to(dev)
        torch.cuda.synchronize()

    def ptrs(self):
        return self.d_text.data_ptr(), len(self.data), self.d_mask.data_ptr()

    def want(self, merges, rank):
        """Chunk by chunk; a single is its id over its whole chunk.  (No chunk is parsed for a number on this route.)"""
        assert 0 not in self.data
        lookup = {tuple(m): 256 + k for k, m in enumerate(np.asarray(merges).tolist())}
        ids = {(s, s + l): i for s, l, i in self.singles}
        toks = []
        for s, e in zip(self.off[:-1].tolist(), self.off[1:].tolist()):
            toks += [[ids[(s, e)], s, e]] if (s, e) in ids else B.encode_chunk(self.data[s:e].tobytes(), s, lookup, rank)
        return (np.array([t[0] for t in toks], dtype=np.uint32),
                np.array([t[1] for t in toks] + [len(self.data)], dtype=np.uint64))


@pytest.mark.parametrize("rank", [False, True], ids=["greedy", "rank"])
def test_singles_from_the_device_split(dev, rank):
    _, merges = B.parse_model(open_golden("taylorswift_gpt4_first_512"))
    names = B.parse_special(read_data("special1.txt"))
    c = MaskCase(dev, read_data("specialtokensample.txt"), names=names)
    assert [i for _, _, i in c.singles] == [100258, 100257]
    want = c.want(merges, rank)
    with mbpe.Encoder(np.array(merges, dtype=np.uint32), rank_order=rank) as enc:
        tokens, doc_tok, boff = enc.encode_endmask(*c.ptrs(), singles=c.singles, byte_off=True)
        check((tokens, boff), want, "split_docs")
        assert doc_tok is None
        for s, l, i in c.singles:                                 # the single's range is its name's occurrence
            j = tokens.tolist().index(i)
            assert (boff[j], boff[j + 1]) == (s, s + l)
        docs = [0, c.singles[0][0], len(c.data)]                  # with document offsets: two queries of one count
        tokens, doc_tok, boff = enc.encode_endmask(*c.ptrs(), singles=c.singles, doc_off=docs, byte_off=True)
        check((tokens, boff), want, "split_docs + documents")
        assert boff[doc_tok.astype(np.int64)].tolist() == docs


def open_golden(name):
    from conftest import read_golden
    return read_golden(name + ".model")


def hand_mask_case(dev, table):
    """End-mask route, by hand: singles as first chunk, as last chunk, two adjacent at output indices 1,023 and 1,024;
    the names are longer than anything their ids decode to (id 258: a merged token; id 70000: beyond the vocabulary)."""
    text, off = with_n_tokens(table, 1022, False)
    names = [b"<|first|>", b"<|at-1023|>", b"<|at-1024|>", b"<|last|>"]
    ids = [258, 70000, 97, 100257]
    tail, tail_off = chunked(6, 200)
    parts = [names[0], text.tobytes(), names[1], names[2], tail.tobytes(), names[3]]
    starts = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    cuts = [starts[1]] + (off[1:].astype(np.int64) + starts[1]).tolist() + [starts[3], starts[4]]
    cuts += (tail_off[1:].astype(np.int64) + starts[4]).tolist() + [starts[6]]
    c = MaskCase(dev, b"".join(parts), [0] + cuts)
    c.singles = [(int(starts[k]), len(parts[k]), i) for k, i in zip((0, 2, 3, 5), ids)]
    return c


@pytest.mark.parametrize("rank", [False, True], ids=["greedy", "rank"])
def test_singles_with_a_hand_built_mask(dev, table, rank):
    c = hand_mask_case(dev, table)
    want = c.want(table, rank)
    if not rank:
        assert want[0][[0, 1023, 1024, -1]].tolist() == [258, 70000, 97, 100257]
    with mbpe.Encoder(table, rank_order=rank) as enc:
        tokens, _, boff = enc.encode_endmask(*c.ptrs(), singles=c.singles, byte_off=True)
        check((tokens, boff), want, "hand-built mask")
        assert enc.encode_endmask(*c.ptrs(), singles=c.singles)[0].tolist() == want[0].tolist()
        # into device memory, 16 bits refused for an id beyond them, then accepted without those singles' ids
        out = torch.zeros(len(c.data), dtype=torch.int32, device=dev)
        d_boff = torch.full((len(c.data) + 1,), -1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        n, _ = enc.encode_endmask(*c.ptrs(), singles=c.singles, out_ptr=out.data_ptr(), cap=len(c.data),
                                  byte_off_ptr=d_boff.data_ptr())
        assert n == len(want[0])
        got = d_boff.cpu().numpy()
        assert got[:n + 1].tolist() == want[1].tolist() and (got[n + 1:] == -1).all()


# ---- pieces and the other call forms -----------------------------------------------------------------------------

def test_pieces_give_the_one_piece_result(dev, table):
    data, off = chunked(21, 64 << 10)
    with mbpe.Encoder(table) as enc:
        whole = enc.encode(data, off, byte_off=True)
        enc.set_option("piece_bytes", 4096)
        check(enc.encode(data, off, byte_off=True), whole, "pieces")
    lens = np.array([len(v) for v in B.vocab_bytes(table.tolist())], dtype=np.uint64)
    assert np.array_equal(whole[1], np.concatenate([[0], np.cumsum(lens[whole[0]], dtype=np.uint64)]).astype(np.uint64))


def raw(enc, text, off, tokens, cap, boff, bits=32, on_device=0, text_on_device=0, text_ptr=None):
    n, passes = ctypes.c_uint64(77), ctypes.c_uint32(77)
    rc = mbpe.lib().mbpe_encoder_encode_byteoff(
        enc._h, ctypes.c_void_p(text_ptr) if text_ptr else (text.ctypes.data if len(text) else None), len(text),
        text_on_device, None if off is None else off.ctypes.data, 0 if off is None else len(off) - 1, tokens, cap, bits,
        on_device, boff, None, ctypes.byref(n), ctypes.byref(passes))
    return rc, n.value


def test_other_call_forms(dev, table):
    data, off = chunked(31, 6000)
    want = B.encode_chunks(data, off, table)
    n = len(want[0])
    with mbpe.Encoder(table) as enc:
        # 16-bit tokens
        tokens, boff = enc.encode(data, off, dtype=np.uint16, byte_off=True)
        assert tokens.dtype == np.uint16
        check((tokens, boff), want, "16 bits")
        # a second call of the same size allocates nothing; neither does a plain one after it, which gives plain results
        before = enc.alloc_count()
        check(enc.encode(data, off, byte_off=True), want, "again")
        assert enc.encode(data, off).tolist() == want[0].tolist()
        assert enc.alloc_count() == before
        # the query: nothing is written to the offsets
        sent = np.full(len(data) + 1, 0x5555555555555555, dtype=np.uint64)
        rc, got_n = raw(enc, data, off, None, 0, sent.ctypes.data)
        assert rc == mbpe.OK and got_n == n and (sent == 0x5555555555555555).all()
        # a cap too small: MBPE_ERR_ARG, the count, and sentinel-filled arrays untouched -- in one piece and in pieces
        out = np.full(len(data), 0xABABABAB, dtype=np.uint32)
        for piece in (0, 1024):
            enc.set_option("piece_bytes", piece)
            rc, got_n = raw(enc, data, off, out.ctypes.data, n - 1, sent.ctypes.data)
            assert rc == mbpe.ERR_ARG and got_n == n
            assert (out == 0xABABABAB).all() and (sent == 0x5555555555555555).all()
        enc.set_option("piece_bytes", 0)
        # the exact cap
        rc, got_n = raw(enc, data, off, out.ctypes.data, n, sent.ctypes.data)
        assert rc == mbpe.OK and out[:n].tolist() == want[0].tolist() and sent[:n + 1].tolist() == want[1].tolist()
        assert (sent[n + 1:] == 0x5555555555555555).all()
        # the empty text: [0] = 0
        sent[:] = 0x5555555555555555
        rc, got_n = raw(enc, data[:0], None, out.ctypes.data, 4, sent.ctypes.data)
        assert rc == mbpe.OK and got_n == 0 and sent[0] == 0 and (sent[1:] == 0x5555555555555555).all()
        # device text, device outputs: the host result
        d_text = torch.from_numpy(data.copy()).to(dev)
        d_out = torch.zeros(len(data), dtype=torch.int32, device=dev)
        d_boff = torch.full((len(data) + 1,), -1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        got_n = enc.encode_device(d_text.data_ptr(), len(data), off, d_out.data_ptr(), len(data),
                                  byte_off_ptr=d_boff.data_ptr())
        assert got_n == n
        assert (d_out.cpu().numpy()[:n].view(np.uint32) & 0x7FFFFFFF).tolist() == want[0].tolist()
        got = d_boff.cpu().numpy()
        assert got[:n + 1].tolist() == want[1].tolist() and (got[n + 1:] == -1).all()
        # offsets that are not 8-byte aligned on the device
        rc, _ = raw(enc, data, off, ctypes.c_void_p(d_out.data_ptr()), len(data), ctypes.c_void_p(d_boff.data_ptr() + 4),
                    on_device=1)
        assert rc == mbpe.ERR_ARG


@pytest.mark.parametrize("merges", [[[97, 98], [99, 100], [97, 98]], [[97, 98], [258, 99]], [[97, 98], [97, 257]]],
                         ids=["pair-twice", "first-side-ahead", "second-side-ahead"])
def test_a_table_that_is_not_a_trained_one(dev, merges):
    merges = np.array(merges, dtype=np.uint32)
    data = np.frombuffer(b"abcdababcd" * 20, dtype=np.uint8)
    with mbpe.Encoder(merges) as enc:
        want = enc.encode(data)
        with pytest.raises(mbpe.MbpeError) as e:
            enc.encode(data, byte_off=True)
        assert e.value.code == mbpe.ERR_ARG and "mbpe_merges_check" in str(e.value)
        d_text = torch.from_numpy(data.copy()).to(dev)
        d_mask = torch.zeros(mbpe.Splitter.mask_bytes(len(data)), dtype=torch.uint8, device=dev)
        d_mask[(len(data) - 1) // 8] = 1 << ((len(data) - 1) % 8)
        torch.cuda.synchronize()
        with pytest.raises(mbpe.MbpeError) as e:
            enc.encode_endmask(d_text.data_ptr(), len(data), d_mask.data_ptr(), byte_off=True)
        assert e.value.code == mbpe.ERR_ARG
        assert enc.encode(data).tolist() == want.tolist()         # the same encoder encodes plainly as before
        assert enc.encode_endmask(d_text.data_ptr(), len(data), d_mask.data_ptr())[0].tolist() == want.tolist()


def test_offsets_beyond_2_32(dev):
    """2^32 + 2^20 bytes of 'a' on the device in chunks of 2^20 bytes, ten doubling merges: 4,195,328 tokens of 1,024
    bytes, in pieces of 2^30 bytes -- the piece base and the totals are 64-bit."""
    n_bytes, chunk = (1 << 32) + (1 << 20), 1 << 20
    merges = np.array([[97, 97]] + [[256 + k, 256 + k] for k in range(9)], dtype=np.uint32)
    n = n_bytes // 1024
    off = np.arange(0, n_bytes + 1, chunk, dtype=np.uint64)
    d_text = torch.full((n_bytes,), 97, dtype=torch.uint8, device=dev)
    d_out = torch.zeros(n, dtype=torch.int32, device=dev)
    d_boff = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    with mbpe.Encoder(merges) as enc:
        enc.set_option("piece_bytes", 1 << 30)
        got = enc.encode_device(d_text.data_ptr(), n_bytes, off, d_out.data_ptr(), n, byte_off_ptr=d_boff.data_ptr())
    assert got == n == 4195328
    assert bool((d_boff == torch.arange(n + 1, dtype=torch.int64, device=dev) * 1024).all())
    assert int(d_boff[-1]) == n_bytes
    assert bool(((d_out & 0x7FFFFFFF) == 265).all())
