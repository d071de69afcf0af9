"""Encode and cut into overlapping windows in one call: Encoder.encode_batch_windows,
Encoder.encode_batch_endmask_windows after Splitter.split_docs and Tokenizer.encode_batch_windows give the matrices of
window_cases.ref_windows over Tokenizer.encode of every text -- with the host split, the device split, the rank
order, through the unique chunks, and with dropout against the oracle of tests/dropout_cases.py."""
import numpy as np
import pytest

import mbpe
import oracle as O
import dropout_cases as D
from byteoff_cases import parse_special
from conftest import read_data, read_golden
from window_cases import ref_windows

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

MODEL = "taylorswift_gpt4_first_512"
SEQ_LEN, STRIDE, PAD, BOS, EOS = 48, 12, 0, 100276, 100257
KW = dict(seq_len=SEQ_LEN, stride=STRIDE, pad_id=PAD, bos_id=BOS, eos_id=EOS)
OUTPUTS = dict(labels=True, positions=True, segments=True, row_doc=True, row_tok0=True)
P, SEED = 0.1, 3


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
    ts = read_data("taylorswift.txt")
    out = [ts[:2500], b"", ts[9000:9100], ts[20000:24001], b"x", ts[40000:40300]]
    if special:
        out.insert(3, read_data("specialtokensample.txt") * 12)       # long enough for several windows
    return out


def want_of(docs, score_once, out_bits=32, **kw):
    """ref_windows over the documents' tokens as the arrays the calls return."""
    k = dict(KW, **kw)
    ref = ref_windows(docs, k["seq_len"], k["stride"], k["bos_id"], k["eos_id"], k["pad_id"], -100, score_once)
    n = len(ref["len"])
    m = lambda key, dt: np.array(ref[key], dtype=np.int64).astype(dt).reshape(n, k["seq_len"])
    return {"ids": m("ids", {32: np.uint32, 64: np.uint64}[out_bits]), "lengths": np.array(ref["len"], dtype=np.uint32),
            "labels": m("labels", {32: np.int32, 64: np.int64}[out_bits]), "positions": m("pos", np.uint32),
            "segments": m("seg", np.uint32), "row_doc": np.array(ref["row_doc"], dtype=np.uint32),
            "row_tok0": np.array(ref["row_tok0"], dtype=np.uint64)}


def same(got, want, what):
    assert sorted(got) == sorted(want), what
    for k in want:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (what, k)


def chunked(pattern, docs):
    """The documents laid end to end, each split on its own -> (buffer, chunk_off, doc_chunk_off)."""
    off, doc_chunk, start = [0], [0], 0
    for d in docs:
        if d:
            off += (start + mbpe.presplit(pattern, np.frombuffer(d, dtype=np.uint8))[1:]).tolist()
        start += len(d)
        doc_chunk.append(len(off) - 1)
    return b"".join(docs), np.array(off, dtype=np.uint64), np.array(doc_chunk, dtype=np.uint64)


def test_tokenizer_routes_give_the_reference_matrices(tok):
    docs = texts()
    tokens = [tok.encode(d).tolist() for d in docs]
    assert any(t >= 100257 for t in tokens[3]) and len(tokens[3]) > 2 * SEQ_LEN
    for score_once in (False, True):
        want = want_of(tokens, score_once)
        for route in (dict(), dict(device_split=True), dict(device_split="unicode"), dict(dedup=True),
                      dict(device_split=True, dedup=True)):
            got = tok.encode_batch_windows(docs, score_once=score_once, **KW, **OUTPUTS, **route)
            same(got, want, (score_once, route))
            assert tok.doc_tok_off.tolist() == np.concatenate([[0], np.cumsum([len(t) for t in tokens])]).tolist()
    # 64-bit ids for an int64 tensor, a subset of the outputs, no bos
    want = want_of(tokens, True, out_bits=64, bos_id=None)
    got = tok.encode_batch_windows(docs, score_once=True, out_bits=64, labels=True, row_doc=True, **dict(KW, bos_id=None))
    same(got, {k: want[k] for k in ("ids", "lengths", "labels", "row_doc")}, "64 bits")
    # the rank order: the reference is the tokenizer's own rank-ordered encode
    ranked = [tok.encode(d, order="rank").tolist() for d in docs]
    for route in (dict(), dict(device_split=True)):
        got = tok.encode_batch_windows(docs, order="rank", **KW, **OUTPUTS, **route)
        same(got, want_of(ranked, False), ("rank", route))


def test_encoder_routes_give_the_reference_matrices(dev, tok, model):
    pattern, merges = model
    docs = texts(special=False)
    tokens = [tok.encode(d).tolist() for d in docs]
    want = want_of(tokens, True)
    buf, off, doc_chunk = chunked(pattern, docs)
    with mbpe.Encoder(merges) as enc:
        got = enc.encode_batch_windows(buf, off, doc_chunk, score_once=True, **KW, **OUTPUTS)
        same(got, want, "encode_batch_windows")
        assert enc.n_tokens == sum(len(t) for t in tokens) and enc.pack_ms() > 0
        # the device form: torch tensors, the row count comes back
        n = len(want["lengths"])
        d_ids, d_lab = (torch.full((n, SEQ_LEN), -1, dtype=torch.int32, device=dev) for _ in range(2))
        d_len, d_doc = (torch.full((n,), -1, dtype=torch.int32, device=dev) for _ in range(2))
        d_tok0 = torch.full((n,), -1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        rows = enc.encode_batch_windows(buf, off, doc_chunk, score_once=True, **KW, out_ptr=d_ids.data_ptr(),
                                        len_ptr=d_len.data_ptr(), cap_rows=n, labels_ptr=d_lab.data_ptr(),
                                        row_doc_ptr=d_doc.data_ptr(), row_tok0_ptr=d_tok0.data_ptr())
        torch.cuda.synchronize()
        assert rows == n
        same({"ids": d_ids.cpu().numpy().view(np.uint32), "labels": d_lab.cpu().numpy(),
              "lengths": d_len.cpu().numpy().view(np.uint32), "row_doc": d_doc.cpu().numpy().view(np.uint32),
              "row_tok0": d_tok0.cpu().numpy().view(np.uint64)},
             {k: want[k] for k in ("ids", "labels", "lengths", "row_doc", "row_tok0")}, "device outputs")
        # a cap one row too small: found after the passes, nothing written, the count reported
        d_ids.fill_(-1)
        torch.cuda.synchronize()
        with pytest.raises(mbpe.MbpeError) as e:
            enc.encode_batch_windows(buf, off, doc_chunk, **KW, out_ptr=d_ids.data_ptr(), len_ptr=d_len.data_ptr(),
                                     cap_rows=n - 1)
        assert e.value.code == mbpe.ERR_ARG and bool((d_ids == -1).all())
    # the end-mask route with a special token: the splitter's text, mask and ranges, nothing on the host in between
    docs = texts()
    tokens = [tok.encode(d).tolist() for d in docs]
    want = want_of(tokens, True)
    specials = parse_special(read_data("special1.txt"))
    names = sorted(specials)
    doc_off = np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.uint64)
    with mbpe.Splitter(pattern) as sp, mbpe.Encoder(merges) as enc:
        n_chunks, ranges = sp.split_docs(b"".join(docs), doc_off, names)
        singles = [(int(s), int(n), specials[names[int(k)]]) for s, n, k in ranges if int(k) != mbpe.SPLIT_RAW]
        assert singles
        mask_ptr, _, text_ptr = sp.endmask()
        got = enc.encode_batch_endmask_windows(text_ptr, int(doc_off[-1]), mask_ptr, singles, doc_off, score_once=True,
                                               **KW, **OUTPUTS)
        same(got, want, "encode_batch_endmask_windows")
        assert enc.doc_tok_off.tolist() == np.concatenate([[0], np.cumsum([len(t) for t in tokens])]).tolist()


def test_dropout_follows_the_oracle(tok, model):
    pattern, merges = model
    docs = texts(special=False)
    buf, off, doc_chunk = chunked(pattern, docs)
    th = D.threshold_of(P)
    stream, end, _, _ = D.reference(buf, off, merges, SEED, th)
    chunk_tok = np.concatenate([[0], np.flatnonzero(end) + 1])
    doc_tok = chunk_tok[doc_chunk.astype(np.int64)]
    tokens = [stream[a:b].tolist() for a, b in zip(doc_tok[:-1], doc_tok[1:])]
    plain = [tok.encode(d, order="rank").tolist() for d in docs]
    assert tokens != plain                                               # the dropout did skip merges
    want = want_of(tokens, True)
    for route in (dict(), dict(device_split=True)):
        got = tok.encode_batch_windows(docs, score_once=True, order="rank", dropout=P, seed=SEED, **KW, **OUTPUTS, **route)
        same(got, want, ("dropout", route))
    with mbpe.Encoder(merges, rank_order=True, dropout=P, seed=SEED) as enc:
        same(enc.encode_batch_windows(buf, off, doc_chunk, score_once=True, **KW, **OUTPUTS), want, "encoder dropout")


def test_repeat_calls_allocate_nothing(model):
    pattern, merges = model
    docs = texts(special=False)
    buf, off, doc_chunk = chunked(pattern, docs)
    doc_off = off[doc_chunk.astype(np.int64)]
    with mbpe.Splitter(pattern) as sp, mbpe.Encoder(merges) as enc:
        sp.split_docs(buf, doc_off, [])
        mask_ptr, _, text_ptr = sp.endmask()
        first = enc.encode_batch_windows(buf, off, doc_chunk, **KW, **OUTPUTS)
        enc.encode_batch_endmask_windows(text_ptr, len(buf), mask_ptr, None, doc_off, **KW, **OUTPUTS)
        before = enc.alloc_count()
        for _ in range(2):
            again = enc.encode_batch_windows(buf, off, doc_chunk, **KW, **OUTPUTS)
            other = enc.encode_batch_endmask_windows(text_ptr, len(buf), mask_ptr, None, doc_off, **KW, **OUTPUTS)
            same(again, first, "repeat")
            same(other, first, "repeat, end mask")
        assert enc.alloc_count() == before
        # fewer documents and a shorter row need nothing new either
        enc.encode_batch_windows(docs[:3], seq_len=32, stride=4, **OUTPUTS)
        assert enc.alloc_count() == before


def test_decode_round_trip(tok):
    docs = texts()
    got = tok.encode_batch_windows(docs, SEQ_LEN, 0, bos_id=BOS, eos_id=EOS, row_doc=True)
    joined = [[] for _ in docs]
    for row, d in enumerate(got["row_doc"]):
        n = int(got["lengths"][row])
        body = got["ids"][row, 1:n].tolist()                            # without bos
        joined[d] += body
    for d in range(len(docs)):
        assert joined[d][-1] == EOS                                      # in the document's last row only
        joined[d].pop()
        assert EOS not in joined[d] or d == 3                            # (the text with the special token has it inside)
    assert tok.decode_batch(joined) == docs
