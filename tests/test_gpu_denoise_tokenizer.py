"""Span corruption through the Tokenizer: encode_batch_denoise equals "encode -> denoise_cases.ref_apply ->
mbpe.pack_tokens / pack_tokens_aux rowwise" over the host split and both device splits, in both orders, with dropout and
with dedup, the sentinels, eos and the decoder start id being special tokens of the model; the query, a cap too small,
device outputs; and fim= / mlm= left on by an earlier call do not leak into it."""
import numpy as np
import pytest

import mbpe
import oracle as O
import denoise_cases as D
from conftest import read_data, read_golden

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

MODEL = "taylorswift_gpt4_first_512"
ENC_LEN, DEC_LEN, PAD = 32, 16, 0
SENT0, N_SENT = 900, 30                                          # ids no merge and no special token has
ROUTES = {
    "host split": {},
    "device split": dict(device_split=True),
    "unicode split": dict(device_split="unicode"),
    "rank order": dict(order="rank"),
    "rank order, device split": dict(order="rank", device_split=True),
    "dropout": dict(order="rank", dropout=0.3, seed=5),
    "dedup": dict(dedup=True),
    "dedup, device split": dict(dedup=True, device_split=True),
}


@pytest.fixture(scope="module")
def tok():
    pattern, _, merges = O.parse_model(read_golden(MODEL + ".model"))
    t = mbpe.Tokenizer(pattern)
    t.set_special_tokens_from_file(read_data("special1.txt"))
    t.set_merges(merges)
    yield t
    t.close()


@pytest.fixture(scope="module")
def special():
    """Two special-token ids of the model's file: eos and the decoder start id."""
    table = [line.split() for line in read_data("special1.txt").decode().splitlines() if line.strip()]
    ids = sorted(int(v) for _, v in table)
    return ids[0], ids[1]


def texts():
    ts = read_data("taylorswift.txt")
    out = [ts[a:a + n] for a, n in ((0, 40), (100, 7), (300, 90), (500, 1), (700, 60), (900, 25), (1200, 110), (1500, 33),
                                    (1800, 75), (2100, 12), (2400, 52))]
    out.insert(2, b"")
    out.insert(5, ts[9000:9400])
    out.append(b"")
    return out


def same(got, want, what):
    assert sorted(got) == sorted(want), (what, sorted(got), sorted(want))
    for k in want:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (what, k)


def composed(token_docs, s, eos, start, out_bits=32, ignore=-100):
    ins, tgs, unit_doc = D.ref_apply(token_docs, s)
    dt = np.uint16 if out_bits == 16 else np.uint32
    fi, oi = D.flat(ins, dt)
    ft, ot = D.flat(tgs, dt)
    kw = dict(out_bits=out_bits, pad_id=PAD, eos_id=eos)
    enc = mbpe.pack_tokens(fi, oi, ENC_LEN, **kw)
    dec = mbpe.pack_tokens_aux(ft, ot, DEC_LEN, bos_id=start, labels=True, ignore_label=ignore, **kw)
    return {"enc_ids": enc[0], "enc_len": enc[1], "dec_ids": dec["ids"], "dec_len": dec["lengths"],
            "dec_labels": dec["labels"], "row_doc": np.array(unit_doc, dtype=np.uint32)}


S = D.spec(D.threshold(0.3), 512, seed=23, doc_base=100, seg=40, sent=SENT0, n_sent=N_SENT)
SPEC = mbpe.denoise_spec(0.3, 2.0, sentinel_id=SENT0, n_sentinels=N_SENT, segment_tokens=40, seed=23, doc_base=100)


def test_the_keyword_spec_is_the_reference_spec():
    assert bytes(SPEC) == bytes(mbpe.DenoiseSpec(S["density"], S["seed"], S["doc_base"], S["mean_q8"], S["seg"],
                                                 S["min_tokens"], S["sent"], S["down"], S["n_sent"]))


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_batch_equals_the_reference_through_pack(tok, special, route):
    eos, start = special
    how = ROUTES[route]
    docs = texts()
    # (with dropout an instance's position runs over the texts laid end to end: the batch's tokens, not each text's own)
    tokens = [t.tolist() for t in tok.encode_batch(docs, **how)]
    if "dropout" not in how:
        assert tokens == [tok.encode(d, device=0, **how).tolist() if d else [] for d in docs]
    want = composed(tokens, S, eos, start)
    n_rows = len(want["row_doc"])
    assert n_rows > len(docs)
    kw = dict(denoise=SPEC, pad_id=PAD, eos_id=eos, decoder_start_id=start, **how)
    got = tok.encode_batch_denoise(docs, ENC_LEN, DEC_LEN, **kw)
    same(got, want, route)
    assert tok.n_tokens == sum(len(t) for t in tokens)
    # the query, a cap too small and device outputs
    assert tok.encode_batch_denoise(docs, ENC_LEN, DEC_LEN, ptrs={}, **kw) == n_rows
    dev = torch.device("cuda", 0)
    t = {k: torch.full(v.shape, -1, dtype=torch.int32, device=dev) for k, v in want.items()}
    ptrs = {k: v.data_ptr() for k, v in t.items()}
    torch.cuda.synchronize()
    with pytest.raises(mbpe.MbpeError) as e:
        tok.encode_batch_denoise(docs, ENC_LEN, DEC_LEN, ptrs=ptrs, cap_rows=n_rows - 1, **kw)
    torch.cuda.synchronize()
    assert e.value.code == mbpe.ERR_ARG and tok.n_rows == n_rows and all(bool((v == -1).all()) for v in t.values())
    assert tok.encode_batch_denoise(docs, ENC_LEN, DEC_LEN, ptrs=ptrs, cap_rows=n_rows, **kw) == n_rows
    torch.cuda.synchronize()
    same({k: v.cpu().numpy().view(np.int32 if k == "dec_labels" else np.uint32) for k, v in t.items()}, want,
         (route, "device outputs"))


def test_other_widths_and_stages_left_on(tok, special):
    eos, start = special
    docs = texts()
    tokens = [t.tolist() for t in tok.encode_batch(docs)]
    kw = dict(denoise=SPEC, pad_id=PAD, decoder_start_id=start)
    # fim= and mlm= are arguments of their calls: a denoise call that follows them is not refused and not transformed
    tok.encode_batch_padded(docs, 16, fim=mbpe.fim_spec(1.0, 0.5, 901, 902, 903))
    tok.encode_batch_aux(docs, 16, labels=True, mlm=mbpe.mlm_spec(0.5, 901, 512))
    same(tok.encode_batch_denoise(docs, ENC_LEN, DEC_LEN, eos_id=eos, **kw), composed(tokens, S, eos, start), "after fim")
    # 64-bit rows; 16-bit rows need every id below 65,536: ids of their own there, the model's specials lie above
    same(tok.encode_batch_denoise(docs, ENC_LEN, DEC_LEN, eos_id=eos, out_bits=64, **kw),
         composed(tokens, S, eos, start, out_bits=64), "64 bits")
    same(tok.encode_batch_denoise(docs, ENC_LEN, DEC_LEN, denoise=SPEC, pad_id=PAD, eos_id=1001, decoder_start_id=None,
                                  out_bits=16, ignore_label=65535),
         composed(tokens, S, 1001, None, out_bits=16, ignore=65535), "16 bits")
    big = mbpe.denoise_spec(0.3, 2.0, sentinel_id=70000, n_sentinels=N_SENT)
    with pytest.raises(mbpe.MbpeError) as e:
        tok.encode_batch_denoise(docs, ENC_LEN, DEC_LEN, denoise=big, out_bits=16, pad_id=PAD, ignore_label=0)
    assert e.value.code == mbpe.ERR_VOCAB


def test_decoding_gives_the_text_back_part_by_part(tok, special):
    """The rows are ids of the model: kept and noise parts decode to the text's own bytes, interleaved."""
    eos, start = special
    docs = [d for d in texts() if d]
    tokens = [t.tolist() for t in tok.encode_batch(docs)]
    s = dict(S, seg=0)
    spec = mbpe.denoise_spec(0.3, 2.0, sentinel_id=SENT0, n_sentinels=N_SENT, seed=23, doc_base=100)
    got = tok.encode_batch_denoise(docs, 512, 512, denoise=spec, pad_id=PAD)
    for d, (text, t) in enumerate(zip(docs, tokens)):
        inp = got["enc_ids"][d, :got["enc_len"][d]].tolist()
        tg = got["dec_ids"][d, :got["dec_len"][d]].tolist()
        assert (inp, tg) == D.ref_unit(s, d, 0, t), d
        back, i, g = [], 0, 1
        while i < len(inp) or g < len(tg):
            while i < len(inp) and not SENT0 - N_SENT < inp[i] <= SENT0:
                back.append(inp[i]); i += 1
            i += 1
            while g < len(tg) and not SENT0 - N_SENT < tg[g] <= SENT0:
                back.append(tg[g]); g += 1
            g += 1
        assert tok.decode_batch([back])[0] == text, d
