"""Masked-LM batches through the Tokenizer and the Encoder: with mlm= the three batch calls equal "encode_batch -> word
ends from the host split -> mlm_cases.ref_apply -> mbpe.pack_* with label_tokens" on every route that feeds the stage
(host split and device split, both orders, dropout, "dedup", special tokens as one-token chunks; through the Encoder a
text cut into pieces -- the Tokenizer has no option that lowers the piece limit, the Encoder has "piece_bytes").  So
bit 31 of the flat stream really is "last token of its word" wherever the stage reads it.  And the stage's own rules:
not together with fim, no whole words from a 16-bit stream, nothing launched or allocated while it is off or at rate 0."""
import ctypes
import re

import numpy as np
import pytest

import mbpe
import oracle as O
import mlm_cases as M
from conftest import read_data, read_golden

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

MODEL = "taylorswift_gpt4_first_512"
SEQ_LEN, PAD, BOS, EOS = 48, 0, 100258, 100257
MASK = 100259                                   # a special token of the model's file stands for [MASK]
AUX = dict(labels=True, positions=True, segments=True)
SPECIALS = [b"<|endoftext|>", b"<|fim_prefix|>", b"<|fim_middle|>", b"<|fim_suffix|>", b"<|endofprompt|>"]
ROUTES = [dict(device_split=False), dict(device_split=True), dict(device_split=False, order="rank"),
          dict(device_split=True, order="rank"), dict(device_split=False, order="rank", dropout=0.3, seed=5),
          dict(device_split=False, dedup=True), dict(device_split=True, dedup=True)]


@pytest.fixture(scope="module")
def tok():
    pattern, _, merges = O.parse_model(read_golden(MODEL + ".model"))
    t = mbpe.Tokenizer(pattern)
    t.set_special_tokens_from_file(read_data("special1.txt"))
    t.set_merges(merges)
    t.split_pattern = pattern
    yield t
    t.close()


def texts():
    ts = read_data("taylorswift.txt")
    out = [ts[a:a + n] for a, n in ((0, 40), (100, 7), (300, 90), (500, 1), (700, 60), (900, 25), (1200, 110), (1500, 33))]
    out.insert(2, b"")
    out.insert(5, ts[9000:9400] + b"<|endoftext|>" + ts[9400:9500])          # a special token inside a text
    out.append(b"<|endofprompt|>" + ts[40:60])
    return out


def chunk_ends(pattern, text):
    """The byte positions behind every chunk of the host split: the text is cut at the special tokens, each of which is
    one chunk, and the rest is split by the pattern (whose matches tile it)."""
    ends, at = set(), 0
    for part in re.split(b"(" + b"|".join(re.escape(s) for s in SPECIALS) + b")", text):
        if part in SPECIALS:
            ends.add(at + len(part))
        elif part:
            ends.update(at + int(e) for e in mbpe.presplit_ranges(pattern, part)[1])
        at += len(part)
    assert not text or at in ends
    return ends


def word_ends(tok, docs, tokens):
    """One flag per token: it is the last of its chunk.  From the tokens' byte lengths and the host split"""
    uniq = sorted({int(t) for d in tokens for t in d})
    size = dict(zip(uniq, (len(b) for b in tok.decode_batch([[u] for u in uniq]))))
    flags = []
    for text, d in zip(docs, tokens):
        ends, at = chunk_ends(tok.split_pattern, text), 0
        for t in d:
            at += size[int(t)]
            flags.append(at in ends)
        assert at == len(text)
    return flags


def same(got, want, what):
    assert sorted(got) == sorted(want), what
    for k in want:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (what, k)


def _c(s):
    """mlm_cases.spec -> mbpe.MlmSpec"""
    return mbpe.MlmSpec(s["select"], s["mask"], s["random"], s["seed"], s["doc_base"], s["mask_id"], s["vocab_n"],
                        s["whole_word"], len(s["protect"]), (ctypes.c_uint32 * 8)(*s["protect"]))


@pytest.mark.parametrize("route", ROUTES, ids=lambda r: ",".join("%s=%s" % kv for kv in r.items()))
def test_batch_calls_equal_the_rule_through_pack(tok, route):
    docs = texts()
    tokens = [t.tolist() for t in tok.encode_batch(docs, **route)]
    ids = [t for d in tokens for t in d]
    off = np.concatenate([[0], np.cumsum([len(d) for d in tokens])]).astype(np.uint64)
    ends = word_ends(tok, docs, tokens)
    assert EOS in ids and 0 < sum(ends) < len(ends)
    for ww in (1, 0):
        s = M.spec(M.threshold(0.4), seed=31, doc_base=1000, mask_id=MASK, vocab_n=256 + 256, whole_word=ww, protect=(EOS,))
        new, tgt = M.ref_apply(s, ids, ends, off)
        new, tgt = np.array(new, dtype=np.uint32), np.array(tgt, dtype=np.uint32)
        assert 0 < (tgt != M.NO_TOKEN).sum() < len(ids) and not (tgt == EOS).any()
        kw = dict(seq_len=SEQ_LEN, pad_id=PAD, bos_id=BOS, eos_id=EOS)
        call = dict(mlm=_c(s), **route)
        for layout in ("padded", "packed"):
            same(tok.encode_batch_aux(docs, layout=layout, **kw, **AUX, **call),
                 mbpe.pack_tokens_aux(new, off, layout=layout, label_tokens=tgt, **kw, **AUX), ("aux", layout, ww))
            assert tok.doc_tok_off.tolist() == off.tolist()
        same(tok.encode_batch_windows(docs, stride=8, score_once=True, row_doc=True, **kw, **AUX, **call),
             mbpe.pack_windows(new, off, stride=8, score_once=True, row_doc=True, label_tokens=tgt, **kw, **AUX), ("windows", ww))
        same(tok.encode_batch_fit(docs, doc_row=True, **kw, **AUX, **call),
             mbpe.pack_fit(new, off, doc_row=True, label_tokens=tgt, **kw, **AUX), ("fit", ww))
    # a call without mlm= is the plain call again
    plain = np.array(ids, dtype=np.uint32)
    same(tok.encode_batch_aux(docs, layout="packed", **kw, **AUX, **route),
         mbpe.pack_tokens_aux(plain, off, layout="packed", **kw, **AUX), "without mlm")


def test_the_rules_of_the_stage(tok):
    docs = texts()
    spec = mbpe.mlm_spec(0.4, MASK, 512, whole_word=True)
    with pytest.raises(mbpe.MbpeError) as e:                     # both stages: never a silent choice
        tok.encode_batch_aux(docs, SEQ_LEN, labels=True, mlm=spec, fim=mbpe.fim_spec(0.5, 0.5, 100258, 100260, 100259))
    assert e.value.code == mbpe.ERR_ARG
    small = mbpe.Tokenizer(tok.split_pattern)
    small.set_merges(np.array([[101, 32], [116, 104]], dtype=np.uint32))
    with pytest.raises(mbpe.MbpeError) as e:                     # a 16-bit stream has no room for the word ends
        small.encode_batch_aux(docs[:2], SEQ_LEN, out_bits=16, labels=True, ignore_label=65535,
                               mlm=mbpe.mlm_spec(0.4, 300, 258, whole_word=True))
    assert e.value.code == mbpe.ERR_ARG
    got = small.encode_batch_aux(docs[:2], SEQ_LEN, out_bits=16, labels=True, ignore_label=65535, mlm=mbpe.mlm_spec(1.0, 300, 258))
    want = small.encode_batch_aux(docs[:2], SEQ_LEN, out_bits=16, ignore_label=65535)
    sel = got["labels"] != 65535                                 # token-level masking of 16-bit ids works
    assert sel.sum() == want["lengths"].sum() and np.array_equal(got["labels"][sel], want["ids"][sel])
    with pytest.raises(mbpe.MbpeError) as e:
        small.encode_batch_aux(docs[:2], SEQ_LEN, out_bits=16, ignore_label=65535, mlm=mbpe.mlm_spec(0.4, 65536, 258))
    assert e.value.code == mbpe.ERR_VOCAB
    small.close()


def test_encoder_stage_pieces_and_allocations():
    """Through the Encoder: chunks are words of a text that is cut into four pieces or more; the stage off or at rate 0
    changes neither the outputs nor alloc_count, and a repeat call with it on allocates nothing."""
    pattern, _, merges = O.parse_model(read_golden(MODEL + ".model"))
    data = np.frombuffer(read_data("taylorswift.txt")[:24000], dtype=np.uint8)
    starts, stops = mbpe.presplit_ranges(pattern, data.tobytes())
    chunk_off = np.concatenate([[0], stops]).astype(np.uint64)
    assert starts[0] == 0 and (starts[1:] == stops[:-1]).all()
    n_chunks = len(chunk_off) - 1
    assert n_chunks > 2500
    doc_chunk_off = np.array([0, 7, 7, 400, 401, 2500, n_chunks], dtype=np.uint64)          # an empty document among them
    kw = dict(seq_len=64, layout="packed", pad_id=PAD, eos_id=EOS, **AUX)
    with mbpe.Encoder(merges) as enc:
        tokens, tok_off = enc.encode(data, chunk_off, offsets=True)
        off = tok_off[doc_chunk_off.astype(np.int64)]
        ends = np.zeros(len(tokens), dtype=bool)
        ends[tok_off[1:][np.diff(tok_off) > 0].astype(np.int64) - 1] = True
        plain = enc.encode_batch_aux(data, chunk_off, doc_chunk_off, **kw)
        plain = enc.encode_batch_aux(data, chunk_off, doc_chunk_off, **kw)
        a = enc.alloc_count()
        enc.set_mlm(mbpe.mlm_spec(0.0, MASK, 512, whole_word=True))          # rate 0: as if it were off
        same(enc.encode_batch_aux(data, chunk_off, doc_chunk_off, **kw), plain, "rate 0")
        assert enc.alloc_count() == a
        s = M.spec(M.threshold(0.3), seed=2, mask_id=MASK, vocab_n=512, whole_word=1)
        new, tgt = M.ref_apply(s, tokens.tolist(), ends.tolist(), off)
        want = mbpe.pack_tokens_aux(np.array(new, dtype=np.uint32), off, label_tokens=np.array(tgt, dtype=np.uint32), **kw)
        enc.set_mlm(mbpe.mlm_spec(0.3, MASK, 512, seed=2, whole_word=True))
        for piece in (0, len(data) // 4):
            enc.set_option("piece_bytes", piece)
            same(enc.encode_batch_aux(data, chunk_off, doc_chunk_off, **kw), want, ("pieces", piece))
            assert enc.kernel_ms() > enc.pack_ms() > 0.0
        enc.set_option("piece_bytes", 0)
        enc.encode_batch_aux(data, chunk_off, doc_chunk_off, **kw)
        b = enc.alloc_count()
        assert b > a                                             # the stage's buffers
        same(enc.encode_batch_aux(data, chunk_off, doc_chunk_off, **kw), want, "repeat")
        assert enc.alloc_count() == b
        enc.set_mlm(None)
        same(enc.encode_batch_aux(data, chunk_off, doc_chunk_off, **kw), plain, "off again")
        assert enc.alloc_count() == b
