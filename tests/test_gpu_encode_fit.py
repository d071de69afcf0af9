"""Encode and pack whole documents by best fit in one call: Encoder.encode_batch_fit and
Encoder.encode_batch_endmask_fit give mbpe.pack_fit of the same encoder's tokens and offsets -- greedy and in rank
order, with and without the unique chunks, with 16-bit ids, without a new allocation on a repeat call -- and
Tokenizer.encode_batch_fit gives every text back whole: the cells of a text, in the order of their positions, are
[bos] + Tokenizer.encode(text) + [eos], with the host split and the device split."""
import numpy as np
import pytest

import mbpe
import oracle as O
from conftest import read_data, read_golden

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

MODEL = "taylorswift_gpt4_first_512"
SEQ_LEN, PAD, BOS, EOS = 48, 0, 100276, 100257
OUTPUTS = dict(labels=True, positions=True, segments=True, cu_seqlens=True, doc_row=True, doc_col=True)


@pytest.fixture(scope="module")
def dev():
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def model():
    pattern, _, merges = O.parse_model(read_golden(MODEL + ".model"))
    return pattern, merges


@pytest.fixture()
def tok(model):
    t = mbpe.Tokenizer(model[0])
    t.set_special_tokens_from_file(read_data("special1.txt"))
    t.set_merges(model[1])
    yield t
    t.close()


def texts(special=True):
    """A dozen short texts, an empty one among them, and two longer than a row."""
    ts = read_data("taylorswift.txt")
    out = [ts[a:a + n] for a, n in ((0, 40), (100, 7), (300, 90), (500, 1), (700, 60), (900, 25), (1200, 110), (1500, 33),
                                    (1800, 75), (2100, 12), (2400, 52))]
    out.insert(2, b"")
    out.insert(5, ts[9000:9400])
    out.append(ts[20000:20700])
    if special:
        out.insert(7, read_data("specialtokensample.txt"))
    return out


def same(got, want, what):
    assert sorted(got) == sorted(want), what
    for k in want:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == w.dtype and np.array_equal(g, w), (what, k)


def shared_rows(segments):
    """Rows that hold more than one document."""
    return sum(len(set(row.tolist()) - {0}) > 1 for row in segments)


def chunked(pattern, docs):
    """The documents laid end to end, each split on its own -> (buffer, chunk_off, doc_chunk_off)."""
    off, doc_chunk, start = [0], [0], 0
    for d in docs:
        if d:
            off += (start + mbpe.presplit(pattern, np.frombuffer(d, dtype=np.uint8))[1:]).tolist()
        start += len(d)
        doc_chunk.append(len(off) - 1)
    return b"".join(docs), np.array(off, dtype=np.uint64), np.array(doc_chunk, dtype=np.uint64)


@pytest.mark.parametrize("rank_order", [False, True])
@pytest.mark.parametrize("dedup", [False, True])
def test_encoder_calls_equal_pack_fit_of_their_tokens(dev, model, rank_order, dedup):
    pattern, merges = model
    docs = texts(special=False)
    buf, off, doc_chunk = chunked(pattern, docs)
    doc_off = off[doc_chunk.astype(np.int64)]
    for out_bits, ignore in ((32, -100), (16, 65535)):
        kw = dict(seq_len=SEQ_LEN, out_bits=out_bits, pad_id=PAD, bos_id=300, eos_id=301, ignore_label=ignore)
        with mbpe.Splitter(pattern) as sp, mbpe.Encoder(merges, rank_order=rank_order, dedup=dedup) as enc:
            tokens, chunk_tok = enc.encode(buf, off, dtype=np.uint16 if out_bits == 16 else np.uint32, offsets=True)
            doc_tok = chunk_tok[doc_chunk.astype(np.int64)]
            want = mbpe.pack_fit(tokens, doc_tok, **kw, **OUTPUTS)
            assert shared_rows(want["segments"]) and (want["segments"] != 0).sum() == len(tokens) + 2 * len(docs)
            got = enc.encode_batch_fit(buf, off, doc_chunk, **kw, **OUTPUTS)
            same(got, want, ("encode_batch_fit", out_bits))
            assert enc.n_tokens == len(tokens) and enc.doc_tok_off.tolist() == doc_tok.tolist() and enc.pack_ms() > 0
            sp.split_docs(buf, doc_off, [])
            mask_ptr, _, text_ptr = sp.endmask()
            other = enc.encode_batch_endmask_fit(text_ptr, len(buf), mask_ptr, None, doc_off, **kw, **OUTPUTS)
            same(other, want, ("encode_batch_endmask_fit", out_bits))
            assert enc.doc_tok_off.tolist() == doc_tok.tolist()
            # a repeat call of no larger size allocates nothing
            before = enc.alloc_count()
            same(enc.encode_batch_fit(buf, off, doc_chunk, **kw, **OUTPUTS), want, "repeat")
            same(enc.encode_batch_endmask_fit(text_ptr, len(buf), mask_ptr, None, doc_off, **kw, **OUTPUTS), want,
                 "repeat, end mask")
            enc.encode_batch_fit(docs[:4], **dict(kw, seq_len=32), **OUTPUTS)
            assert dedup or enc.alloc_count() == before                   # (the deduper's own buffers are its own matter)


def test_encoder_device_outputs_and_cap(dev, model):
    pattern, merges = model
    docs = texts(special=False)
    buf, off, doc_chunk = chunked(pattern, docs)
    kw = dict(seq_len=SEQ_LEN, pad_id=PAD, eos_id=301)
    with mbpe.Encoder(merges) as enc:
        want = enc.encode_batch_fit(buf, off, doc_chunk, **kw, **OUTPUTS)
        n, n_docs = len(want["lengths"]), len(docs)
        d_ids, d_lab, d_seg = (torch.full((n, SEQ_LEN), -1, dtype=torch.int32, device=dev) for _ in range(3))
        d_len = torch.full((n,), -1, dtype=torch.int32, device=dev)
        d_row = torch.full((n_docs,), -1, dtype=torch.int64, device=dev)
        d_col = torch.full((n_docs,), -1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        rows, cu, longest = enc.encode_batch_fit(buf, off, doc_chunk, **kw, cu_seqlens=True, out_ptr=d_ids.data_ptr(),
                                                 len_ptr=d_len.data_ptr(), cap_rows=n, labels_ptr=d_lab.data_ptr(),
                                                 seg_ptr=d_seg.data_ptr(), doc_row_ptr=d_row.data_ptr(),
                                                 doc_col_ptr=d_col.data_ptr())
        torch.cuda.synchronize()
        assert rows == n and cu.tolist() == want["cu_seqlens"].tolist() and longest == want["max_seqlen"]
        same({"ids": d_ids.cpu().numpy().view(np.uint32), "labels": d_lab.cpu().numpy(),
              "segments": d_seg.cpu().numpy().view(np.uint32), "lengths": d_len.cpu().numpy().view(np.uint32),
              "doc_row": d_row.cpu().numpy().view(np.uint64), "doc_col": d_col.cpu().numpy().view(np.uint32)},
             {k: want[k] for k in ("ids", "labels", "segments", "lengths", "doc_row", "doc_col")}, "device outputs")
        # cu_seqlens are the runs of equal (row, segment) of the flattened matrix, pad runs included
        seg = want["segments"].reshape(-1)
        cuts = [0] + [c for c in range(1, len(seg)) if seg[c] != seg[c - 1] or c % SEQ_LEN == 0] + [len(seg)]
        assert want["cu_seqlens"].tolist() == cuts
        # a cap one row too small: found after the passes, nothing written, the count reported
        d_ids.fill_(-1)
        d_row.fill_(-1)
        torch.cuda.synchronize()
        with pytest.raises(mbpe.MbpeError) as e:
            enc.encode_batch_fit(buf, off, doc_chunk, **kw, out_ptr=d_ids.data_ptr(), len_ptr=d_len.data_ptr(),
                                 cap_rows=n - 1, doc_row_ptr=d_row.data_ptr())
        assert e.value.code == mbpe.ERR_ARG and bool((d_ids == -1).all()) and bool((d_row == -1).all())


def test_tokenizer_gives_every_text_back_whole(tok):
    docs = texts()
    tokens = [tok.encode(d).tolist() for d in docs]
    assert any(t >= 100257 for t in tokens[7]) and sum(len(t) + 2 > SEQ_LEN for t in tokens) >= 2
    kw = dict(seq_len=SEQ_LEN, pad_id=PAD, bos_id=BOS, eos_id=EOS)
    host = tok.encode_batch_fit(docs, **kw, **OUTPUTS)
    assert tok.doc_tok_off.tolist() == np.concatenate([[0], np.cumsum([len(t) for t in tokens])]).tolist()
    assert shared_rows(host["segments"])
    seg, pos, ids, lab = (host[k].reshape(-1) for k in ("segments", "positions", "ids", "labels"))
    for d, t in enumerate(tokens):
        E = [BOS] + t + [EOS]
        cells = np.flatnonzero(seg == d + 1)
        cells = cells[np.argsort(pos[cells], kind="stable")]
        assert pos[cells].tolist() == list(range(len(E))) and ids[cells].tolist() == E, d
        assert lab[cells].tolist() == E[1:] + [-100], d
        if len(E) <= SEQ_LEN:                                             # whole, in one row, contiguous
            assert cells.tolist() == list(range(cells[0], cells[0] + len(E))) and cells[0] // SEQ_LEN == cells[-1] // SEQ_LEN
        first_of_last = cells[(len(E) - 1) // SEQ_LEN * SEQ_LEN]
        assert (host["doc_row"][d], host["doc_col"][d]) == (first_of_last // SEQ_LEN, first_of_last % SEQ_LEN)
    assert (ids[seg == 0] == PAD).all() and (lab[seg == 0] == -100).all()
    assert host["lengths"].tolist() == (host["segments"] != 0).sum(axis=1).tolist()
    for route in (dict(device_split=True), dict(dedup=True), dict(device_split=True, dedup=True)):
        same(tok.encode_batch_fit(docs, **kw, **OUTPUTS, **route), host, route)
    # the rank order: the tokenizer's own rank-ordered encode, through pack_fit
    ranked = [tok.encode(d, order="rank") for d in docs]
    off = np.concatenate([[0], np.cumsum([len(t) for t in ranked])]).astype(np.uint64)
    want = mbpe.pack_fit(np.concatenate(ranked).astype(np.uint32), off, **kw, **OUTPUTS)
    for route in (dict(), dict(device_split=True)):
        same(tok.encode_batch_fit(docs, order="rank", **kw, **OUTPUTS, **route), want, ("rank", route))
