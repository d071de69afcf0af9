"""The encoder's option "dedup" (csrc/encode.hip, csrc/expand.hip): dedup on the device, the merge passes over the unique
chunks, and the expansion that writes every chunk's tokens to its place.

The expected tokens are the Python loops chunk by chunk: encode_rank_cases.rank_loop_chunk in rank order and the
oracle's greedy loop (oracle_encode of tests/test_gpu_encode_spans.py) in the default order; a chunk that is one token
by rule is that token.  In addition every result must equal the same encoder without the option.  That the route ran is
shown by dedup_stats(), which must equal the chunk, unique and byte counts of dedup_cases.dedup exactly, and by
pass_tokens()[0], the unique bytes.  The shapes (tests/expand_cases.py) lie around the expansion's spans of 1,024 chunks
and its 16-byte pieces; with the table NEVER a chunk's token count is its byte count."""
import functools

import numpy as np
import pytest

import mbpe
import oracle as O
import dedup_cases as D
import encode_rank_cases as R
import expand_cases as X
from conftest import read_data, read_golden
from test_bruteforce_cpu import text_to_vector
from test_gpu_encode_spans import oracle_encode
from test_gpu_encode_split import Case as DeviceCase
from test_gpu_encoder import one_byte_chunks
from test_gpu_pack import ref_pack
from test_gpu_pack_aux import ref_aux

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

END = 0x80000000
SENTINEL = 0x5A5A5A5A
ORDERS = ("greedy", "rank")
TABLES = {"never": X.NEVER, "real": O.parse_model(read_golden("taylorswift_gpt4_lexical_512.model"))[2]}


@pytest.fixture(scope="module")
def dev():
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def _shapes():
    s = {"none": ([], None), "one": ([b"hello"], None), "equal-700": (X.equal_chunks(), None),
         "distinct-600": (X.distinct_chunks(), None), "long": (X.long_chunks(), None), "nul": (X.nul_chunks(), None)}
    for n in (1023, 1024, 1025, 4095, 4096, 4097):
        s["edge-%d" % n] = (X.edge_chunks(n), None)
    for r in range(8):
        s["residue-%d" % r] = (X.residue_chunks(r), None)
    chunks = X.edge_chunks(1500, seed=3)
    s["empty-chunks"] = (chunks, X.with_empty_chunks(chunks)[1])
    return s


SHAPES = _shapes()


def shape(name):
    """-> (text uint8, chunk_off uint64, the chunks that are not empty)"""
    chunks, off = SHAPES[name]
    data, plain_off = D.join(chunks)
    return data, (plain_off if off is None else off), chunks


@functools.lru_cache(maxsize=None)
def reference(name, table, order, singles=()):
    """The loops, chunk by chunk -> (tokens, token offsets of the chunks, True on every chunk's last token).  singles:
    ((chunk index, id), ..): chunks that are one token whatever their bytes."""
    data, off, _ = shape(name)
    merges = TABLES[table]
    pieces = R.chunks_of(data, off)
    if order == "rank":
        lookup = R.lookup_of(merges)
        per = [rank_tokens(ch, lookup) for ch in pieces]
    else:
        tok, lens = oracle_encode(R.RankCase(data, off, merges, name))
        cuts = np.concatenate([[0], np.cumsum(lens)])
        per = [tok[int(a):int(b)].tolist() for a, b in zip(cuts[:-1], cuts[1:])]
    for c, i in singles:
        per[c] = [i]
    tok_off = np.concatenate([[0], np.cumsum([len(p) for p in per])]).astype(np.uint64)
    tokens = np.array([t for p in per for t in p], dtype=np.uint32)
    end = np.zeros(len(tokens), dtype=bool)
    end[tok_off[1:][np.diff(tok_off.astype(np.int64)) > 0].astype(np.int64) - 1] = True
    for a in (tokens, tok_off, end):
        a.setflags(write=False)
    return tokens, tok_off, end


def rank_tokens(chunk, lookup):
    return R.rank_loop_chunk(text_to_vector(chunk), lookup)[0] if chunk else []


def encoders(table, order):
    return (mbpe.Encoder(TABLES[table], rank_order=order == "rank", dedup=True),
            mbpe.Encoder(TABLES[table], rank_order=order == "rank"))


def stats_are_dedups(enc, chunks, max_chunk_bytes=D.MAX_CHUNK_BYTES):
    u, _, _ = D.dedup(chunks, max_chunk_bytes)
    st = enc.dedup_stats()
    want = (len(chunks), len(u), sum(len(c) for c in u))
    assert (st["n_chunks"], st["n_unique"], st["n_unique_bytes"]) == want
    if chunks:
        assert enc.pass_tokens()[0] == want[2] and st["n_unique_tokens"] > 0
    return st


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("table", sorted(TABLES))
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shapes(dev, name, table, order):
    data, off, chunks = shape(name)
    want, want_off, want_end = reference(name, table, order)
    if table == "never" and name != "nul":
        assert len(want) == len(data)                       # a chunk's token count is its byte count
    dd, plain = encoders(table, order)
    with dd, plain:
        # host text, host output, with the chunks' token offsets; the same without the option
        got, got_off = dd.encode(data, off, offsets=True)
        assert np.array_equal(got, want) and np.array_equal(got_off, want_off)
        stats_are_dedups(dd, chunks)
        other, other_off = plain.encode(data, off, offsets=True)
        assert np.array_equal(got, other) and np.array_equal(got_off, other_off) and dd.n_passes <= plain.n_passes
        with pytest.raises(mbpe.MbpeError) as e:
            plain.dedup_stats()
        assert e.value.code == mbpe.ERR_STATE
        assert np.array_equal(dd.encode(data, off), want)
        assert np.array_equal(dd.encode(data, off, dtype=np.uint16), want.astype(np.uint16))
        # device text, device output: bit 31 on every chunk's last token, nothing beyond the count
        text = torch.from_numpy(np.concatenate([data, np.zeros(16, dtype=np.uint8)])).to(dev)
        n = len(want)
        out = torch.full((n + 5,), SENTINEL, dtype=torch.int32, device=dev)
        cnt, off_dev = dd.encode_device(text.data_ptr(), len(data), off, out.data_ptr(), n, offsets=True)
        raw = out.cpu().numpy().view(np.uint32)
        assert cnt == n and np.array_equal(off_dev, want_off)
        assert np.array_equal(raw[:n] & np.uint32(END - 1), want) and (raw[n:] == SENTINEL).all()
        assert np.array_equal((raw[:n] & np.uint32(END)) != 0, want_end)
        stats_are_dedups(dd, chunks)
        # 16-bit device output that starts at an odd element: any even address
        out16 = torch.full((n + 9,), 0x5A5A, dtype=torch.int16, device=dev)
        cnt = dd.encode_device(text.data_ptr(), len(data), off, out16.data_ptr() + 2, n, token_bits=16)
        raw16 = out16.cpu().numpy().view(np.uint16)
        assert cnt == n and np.array_equal(raw16[1:n + 1], want.astype(np.uint16))
        assert raw16[0] == 0x5A5A and (raw16[n + 1:] == 0x5A5A).all()
        # device text that is not 16-byte aligned
        if len(data):
            shifted = torch.from_numpy(np.concatenate([np.zeros(3, dtype=np.uint8), data, np.zeros(16, dtype=np.uint8)])).to(dev)
            out.fill_(SENTINEL)
            assert dd.encode_device(shifted.data_ptr() + 3, len(data), off, out.data_ptr(), n) == n
            assert np.array_equal(out.cpu().numpy().view(np.uint32)[:n] & np.uint32(END - 1), want)
        # the query, and a cap one below the count: MBPE_ERR_ARG, nothing written, the count reported
        assert dd.encode_device(text.data_ptr(), len(data), off, 0, 0) == n
        if n:
            out.fill_(SENTINEL)
            cnt_box = []
            with pytest.raises(mbpe.MbpeError) as e:
                cnt_box.append(dd.encode_device(text.data_ptr(), len(data), off, out.data_ptr(), n - 1))
            assert e.value.code == mbpe.ERR_ARG and (out.cpu().numpy().view(np.uint32) == SENTINEL).all()
            assert dd.dedup_stats()["n_chunks"] == len(chunks)


def test_one_byte_chunks():
    """3,077 chunks of one byte, b"a" and b"b" in turn (one_byte_chunks of tests/test_gpu_encoder.py): two unique
    chunks, every chunk kept, and the chunks' token offsets are the byte offsets."""
    c = one_byte_chunks()
    want, lens = oracle_encode(c)
    want_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    assert np.array_equal(want, c.data) and np.array_equal(want_off, c.chunk_off)      # (what the oracle says of it)
    with mbpe.Encoder(c.merges, dedup=True) as enc:
        got, off = enc.encode(c.data, c.chunk_off, offsets=True)
        assert np.array_equal(got, want) and np.array_equal(off, want_off)
        st = enc.dedup_stats()
        assert (st["n_chunks"], st["n_unique"], st["n_unique_bytes"]) == (len(c.data), 2, 2)


def test_too_small_reports_the_count(dev):
    """The C-ABI's n_out of a cap that is too small (the Python wrapper raises before it returns it)."""
    import ctypes
    data, off, _ = shape("edge-1025")
    want = reference("edge-1025", "never", "greedy")[0]
    out = np.full(len(want), SENTINEL, dtype=np.uint32)
    n = ctypes.c_uint64()
    with mbpe.Encoder(X.NEVER, dedup=True) as enc:
        rc = mbpe.lib().mbpe_encoder_encode(enc._h, data.ctypes.data, len(data), 0, off.ctypes.data, len(off) - 1,
                                            out.ctypes.data, len(want) - 1, 32, 0, None, ctypes.byref(n), None)
        assert rc == mbpe.ERR_ARG and n.value == len(want) and (out == SENTINEL).all()
        assert np.array_equal(enc.encode(data, off), want)


@pytest.mark.parametrize("order", ORDERS)
def test_a_long_chunk_three_times(order):
    data, off, chunks = shape("long")
    want = reference("long", "real", order)[0]
    dd, plain = encoders("real", order)
    with dd, plain:
        assert np.array_equal(dd.encode(data, off), want)
        st = stats_are_dedups(dd, chunks)
        assert st["n_unique"] == 5                          # above 256 bytes: the three copies pass through
        dd.set_option("dedup_max_chunk_bytes", 8192)
        assert np.array_equal(dd.encode(data, off), want)
        st = stats_are_dedups(dd, chunks, 8192)
        assert st["n_unique"] == 3                          # ... and now they are expanded from one run
        assert np.array_equal(plain.encode(data, off), want)
        for bad in (-1, 1 << 31):
            with pytest.raises(mbpe.MbpeError) as e:
                dd.set_option("dedup_max_chunk_bytes", bad)
            assert e.value.code == mbpe.ERR_ARG
        with pytest.raises(mbpe.MbpeError) as e:
            dd.set_option("dedup", 2)
        assert e.value.code == mbpe.ERR_ARG


def test_vocab_error():
    chunks = [b"ab", b"\x0070000", b"ab", b"\x0070000"]
    data, off = D.join(chunks)
    dd, plain = encoders("never", "greedy")
    with dd, plain:
        for enc in (dd, plain):
            with pytest.raises(mbpe.MbpeError) as e:
                enc.encode(data, off, dtype=np.uint16)
            assert e.value.code == mbpe.ERR_VOCAB
        assert dd.encode(data, off).tolist() == [97, 98, 70000, 97, 98, 70000] == plain.encode(data, off).tolist()


@pytest.mark.parametrize("order", ORDERS)
def test_endmask_with_singles_and_documents(dev, order):
    """The end-mask call: the singles' bytes are ordinary text that is one token by the caller's word."""
    words = X.edge_chunks(2300, seed=9)
    name_a, name_b = b"<|endoftext|>", b"<|pad|>"
    single_ids = {}
    chunks = []
    for i, w in enumerate(words):
        chunks.append(w)
        if i % 97 == 5:
            single_ids[len(chunks)] = 100257
            chunks.append(name_a)
        if i % 211 == 0:
            single_ids[len(chunks)] = 7
            chunks.append(name_b)
    SHAPES["endmask-" + order] = (chunks, None)
    data, off, _ = shape("endmask-" + order)
    singles = tuple(sorted(single_ids.items()))
    want, want_off, _ = reference("endmask-" + order, "real", order, singles)
    rows = [(int(off[c]), len(chunks[c]), i) for c, i in singles]
    rng = np.random.default_rng(4)
    docs = np.unique(np.concatenate([[0, len(chunks)], rng.integers(0, len(chunks), size=60)])).astype(np.uint64)
    d = DeviceCase(dev, data, off, docs)
    dd, plain = encoders("real", order)
    with dd, plain:
        got, doc_tok = dd.encode_endmask(*d.ptrs(), singles=rows, doc_off=d.doc_off)
        assert np.array_equal(got, want) and np.array_equal(doc_tok, want_off[docs.astype(np.int64)])
        stats_are_dedups(dd, chunks)
        other, other_doc = plain.encode_endmask(*d.ptrs(), singles=rows, doc_off=d.doc_off)
        assert np.array_equal(got, other) and np.array_equal(doc_tok, other_doc)
        # every chunk a document; the query; 16 bits where the ids fit
        got, doc_tok = dd.encode_endmask(*d.ptrs(), singles=rows, doc_off=off)
        assert np.array_equal(got, want) and np.array_equal(doc_tok, want_off)
        n, doc_tok = dd.encode_endmask(*d.ptrs(), singles=rows, doc_off=d.doc_off, query=True)
        assert n == len(want) and np.array_equal(doc_tok, want_off[docs.astype(np.int64)])
        with pytest.raises(mbpe.MbpeError) as e:
            dd.encode_endmask(*d.ptrs(), singles=rows, dtype=np.uint16)
        assert e.value.code == mbpe.ERR_VOCAB
        small = [(s, ln, 300 if i == 100257 else i) for s, ln, i in rows]
        got16, _ = dd.encode_endmask(*d.ptrs(), singles=small, dtype=np.uint16)
        assert np.array_equal(got16, np.where(want == 100257, 300, want).astype(np.uint16))
        # left on the device, with a cap that is too small first
        out = torch.full((len(want) + 3,), SENTINEL, dtype=torch.int32, device=dev)
        with pytest.raises(mbpe.MbpeError) as e:
            dd.encode_endmask(*d.ptrs(), singles=rows, doc_off=d.doc_off, out_ptr=out.data_ptr(), cap=len(want) - 1)
        assert e.value.code == mbpe.ERR_ARG and (out.cpu().numpy().view(np.uint32) == SENTINEL).all()
        n, _ = dd.encode_endmask(*d.ptrs(), singles=rows, doc_off=d.doc_off, out_ptr=out.data_ptr(), cap=len(want))
        raw = out.cpu().numpy().view(np.uint32)
        assert n == len(want) and np.array_equal(raw[:n] & np.uint32(END - 1), want) and (raw[n:] == SENTINEL).all()
        # the batch form of the same documents
        for seq_len in (8, 64):
            for layout in ("padded", "packed"):
                kw = dict(seq_len=seq_len, layout=layout, pad_id=3000, bos_id=None if layout == "packed" else 3001,
                          eos_id=3002)
                want_ids, want_len = ref_pack(want, want_off[docs.astype(np.int64)], seq_len, layout, 32, pad=3000,
                                              bos=kw["bos_id"], eos=3002)
                ids, lengths = dd.encode_batch_endmask(*d.ptrs(), rows, d.doc_off, **kw)
                assert np.array_equal(ids, want_ids) and np.array_equal(lengths, want_len), (seq_len, layout)
                assert np.array_equal(dd.doc_tok_off, want_off[docs.astype(np.int64)])
                ids2, lengths2 = plain.encode_batch_endmask(*d.ptrs(), rows, d.doc_off, **kw)
                assert np.array_equal(ids, ids2) and np.array_equal(lengths, lengths2)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name", ["edge-4097", "empty-chunks", "nul"])
def test_batch_calls(name, order):
    data, off, chunks = shape(name)
    want, want_off, _ = reference(name, "real", order)
    n_chunks = len(off) - 1
    rng = np.random.default_rng(9)
    docs = np.unique(np.concatenate([[0, n_chunks], rng.integers(0, n_chunks, size=40)])).astype(np.uint64)
    doc_tok = want_off[docs.astype(np.int64)]
    dd, plain = encoders("real", order)
    with dd, plain:
        for seq_len in (8, 64):
            for layout in ("padded", "packed"):
                kw = dict(seq_len=seq_len, layout=layout, pad_id=3000, bos_id=None if layout == "packed" else 3001,
                          eos_id=3002)
                ref_kw = dict(pad=3000, bos=kw["bos_id"], eos=3002)
                want_ids, want_len = ref_pack(want, doc_tok, seq_len, layout, 32, **ref_kw)
                ids, lengths = dd.encode_batch(data, off, docs, **kw)
                assert np.array_equal(ids, want_ids) and np.array_equal(lengths, want_len), (seq_len, layout)
                assert dd.n_tokens == len(want)
                stats_are_dedups(dd, chunks)
                got = dd.encode_batch_aux(data, off, docs, labels=True, positions=True, segments=True, **kw)
                ref = dict(zip(("ids", "lengths", "labels", "positions", "segments"),
                               ref_aux(want, doc_tok, seq_len, layout, 32, **ref_kw)))
                assert np.array_equal(dd.doc_tok_off, doc_tok)
                other = plain.encode_batch_aux(data, off, docs, labels=True, positions=True, segments=True, **kw)
                for k in ref:
                    assert np.array_equal(np.asarray(got[k]).view(ref[k].dtype), ref[k]), (seq_len, layout, k)
                    assert np.array_equal(got[k], other[k]), (seq_len, layout, k)


def test_errors_leave_the_encoder_usable():
    data, off, _ = shape("edge-1023")
    want = reference("edge-1023", "real", "rank")[0]
    with mbpe.Encoder(TABLES["real"], rank_order=True, dedup=True) as enc:
        assert np.array_equal(enc.encode(data, off), want)
        enc.set_dropout(0.25, seed=3)
        with pytest.raises(mbpe.MbpeError) as e:
            enc.encode(data, off)
        assert e.value.code == mbpe.ERR_ARG and "dropout" in str(e.value)
        with pytest.raises(mbpe.MbpeError) as e:
            enc.encode_batch(data, off, None, seq_len=8)
        assert e.value.code == mbpe.ERR_ARG
        enc.set_dropout(0.0)
        assert np.array_equal(enc.encode(data, off), want)
        with pytest.raises(mbpe.MbpeError) as e:
            enc.encode(data, off, byte_off=True)
        assert e.value.code == mbpe.ERR_ARG and "byte offsets" in str(e.value)
        assert np.array_equal(enc.encode(data, off), want)
        # without the option the same encoder computes both again
        enc.set_option("dedup", 0)
        tokens, boff = enc.encode(data, off, byte_off=True)
        assert np.array_equal(tokens, want) and boff[-1] == len(data)
        with pytest.raises(mbpe.MbpeError) as e:
            enc.dedup_stats()
        assert e.value.code == mbpe.ERR_STATE


def test_unique_text_above_the_piece_limit():
    data, off, _ = shape("distinct-600")
    want = reference("distinct-600", "real", "greedy")[0]
    with mbpe.Encoder(TABLES["real"], dedup=True) as enc:
        enc.set_option("piece_bytes", 1000)                  # the unique text has 1,800 bytes
        with pytest.raises(mbpe.MbpeError) as e:
            enc.encode(data, off)
        assert e.value.code == mbpe.ERR_OOM and "1800" in str(e.value)
        enc.set_option("piece_bytes", 0)
        assert np.array_equal(enc.encode(data, off), want)
        # 700 equal chunks are 1,400 bytes of text and 2 unique bytes: they fit where the text itself would not
        data, off, _ = shape("equal-700")
        enc.set_option("piece_bytes", 1000)
        assert np.array_equal(enc.encode(data, off), reference("equal-700", "real", "greedy")[0])


def test_repeat_call_allocates_nothing(dev):
    data, off, _ = shape("edge-4097")
    small, small_off, _ = shape("edge-1023")
    with mbpe.Encoder(TABLES["real"], rank_order=True, dedup=True) as enc:
        first, first_off = enc.encode(data, off, offsets=True)
        before = enc.alloc_count()
        enc.encode(small, small_off, offsets=True)
        again, again_off = enc.encode(data, off, offsets=True)
        assert enc.alloc_count() == before
        assert np.array_equal(first, again) and np.array_equal(first_off, again_off)
        assert enc.kernel_ms() > 0 and enc.dedup_stats()["expand_ms"] > 0
    # and without the option nothing of the route exists
    with mbpe.Encoder(TABLES["real"], rank_order=True) as a, mbpe.Encoder(TABLES["real"], rank_order=True) as b:
        a.encode(data, off)
        b.set_option("dedup", 1)
        b.set_option("dedup", 0)
        b.encode(data, off)
        assert a.alloc_count() == b.alloc_count()


@pytest.fixture(scope="module")
def shakespeare():
    data = np.frombuffer(read_data("shakespeare.txt"), dtype=np.uint8)
    off = mbpe.presplit(O.GPT4_SPLIT_PATTERN, data)
    merges = O.parse_model(read_golden("shakespeare_gpt4_lexical_512.model"))[2]
    return data, off, merges


@pytest.mark.parametrize("order", ORDERS)
def test_shakespeare(shakespeare, order):
    data, off, merges = shakespeare
    chunks = D.chunks_of(data, off)
    if order == "rank":
        with mbpe.Trainer(0) as tr:
            trained = tr.train(data, 512, off, conflict_resolution=1)[0]
            want, _ = tr.stream()
        assert np.array_equal(np.asarray(trained).reshape(-1, 2), np.asarray(merges).reshape(-1, 2))
        want = want & np.uint32(END - 1)
    else:
        want = O.encode_chunks(data, off, merges)
    with mbpe.Encoder(merges, rank_order=order == "rank", dedup=True) as dd, \
            mbpe.Encoder(merges, rank_order=order == "rank") as plain:
        got, got_off = dd.encode(data, off, offsets=True)
        assert np.array_equal(got, want)
        st = stats_are_dedups(dd, chunks)
        other, other_off = plain.encode(data, off, offsets=True)
        assert np.array_equal(got, other) and np.array_equal(got_off, other_off)
        print(order, st, "kernel ms", dd.kernel_ms(), "against", plain.kernel_ms(), "without")
