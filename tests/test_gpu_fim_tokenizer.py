"""Fill-in-the-middle through the Tokenizer: with fim= the four batch calls equal "encode_batch -> fim_cases.ref_apply
-> mbpe.pack_*" with the host split and with the device split, the sentinels being special tokens of the model; and
decoding the transformed tokens gives the sentinels' names around the texts' own bytes, in PSM / SPM order."""
import numpy as np
import pytest

import mbpe
import oracle as O
import fim_cases as F
from conftest import read_data, read_golden

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

MODEL = "taylorswift_gpt4_first_512"
SEQ_LEN, PAD, EOS = 48, 0, 100257
NAMES = {"pre": b"<|fim_prefix|>", "suf": b"<|fim_suffix|>", "mid": b"<|fim_middle|>"}
AUX = dict(labels=True, positions=True, segments=True)


@pytest.fixture(scope="module")
def tok():
    pattern, _, merges = O.parse_model(read_golden(MODEL + ".model"))
    t = mbpe.Tokenizer(pattern)
    t.set_special_tokens_from_file(read_data("special1.txt"))
    t.set_merges(merges)
    yield t
    t.close()


@pytest.fixture(scope="module")
def ids():
    """The sentinel ids: the special tokens of the model's file."""
    table = dict(line.split() for line in read_data("special1.txt").decode().splitlines() if line.strip())
    return {k: int(table[v.decode()]) for k, v in NAMES.items()}


def texts():
    ts = read_data("taylorswift.txt")
    out = [ts[a:a + n] for a, n in ((0, 40), (100, 7), (300, 90), (500, 1), (700, 60), (900, 25), (1200, 110), (1500, 33),
                                    (1800, 75), (2100, 12), (2400, 52))]
    out.insert(2, b"")
    out.insert(5, ts[9000:9400])
    return out


def same(got, want, what):
    if isinstance(want, tuple):
        got, want = dict(zip("ab", got)), dict(zip("ab", want))
    assert sorted(got) == sorted(want), what
    for k in want:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (what, k)


@pytest.fixture(scope="module")
def case(tok, ids):
    """The texts, their tokens, the rule's parameters and the transformed documents: computed once."""
    docs = texts()
    tokens = [t.tolist() for t in tok.encode_batch(docs)]
    s = F.spec(F.threshold(0.8), F.threshold(0.5), seed=23, doc_base=100, pre=ids["pre"], suf=ids["suf"], mid=ids["mid"])
    new = F.ref_apply(tokens, s)
    plan = F.ref_plan([len(t) for t in tokens], s)
    assert {F.NONE, F.PSM, F.SPM} <= set(plan[1])
    spec = mbpe.fim_spec(0.8, 0.5, ids["pre"], ids["suf"], ids["mid"], seed=23, doc_base=100)
    return docs, tokens, s, new, plan, spec


@pytest.mark.parametrize("device_split", [False, True])
def test_batch_calls_equal_the_reference_through_pack(tok, case, device_split):
    docs, tokens, s, new, plan, spec = case
    flat, off = F.flat(new)
    kw = dict(seq_len=SEQ_LEN, pad_id=PAD, eos_id=EOS)
    route = dict(device_split=device_split, fim=spec)
    for layout in ("padded", "packed"):
        same(tok.encode_batch_padded(docs, layout=layout, **kw, **route), mbpe.pack_tokens(flat, off, layout=layout, **kw),
             (layout, device_split))
        mode, cuts = tok.fim_info()
        assert mode.tolist() == plan[1] and cuts.tolist() == plan[2]
        same(tok.encode_batch_aux(docs, layout=layout, **kw, **AUX, **route),
             mbpe.pack_tokens_aux(flat, off, layout=layout, **kw, **AUX), ("aux", layout, device_split))
        assert tok.doc_tok_off.tolist() == plan[0]
    same(tok.encode_batch_windows(docs, stride=8, row_doc=True, **kw, **AUX, **route),
         mbpe.pack_windows(flat, off, stride=8, row_doc=True, **kw, **AUX), ("windows", device_split))
    assert tok.doc_tok_off.tolist() == plan[0]
    same(tok.encode_batch_fit(docs, doc_row=True, doc_col=True, cu_seqlens=True, **kw, **AUX, **route),
         mbpe.pack_fit(flat, off, doc_row=True, doc_col=True, cu_seqlens=True, **kw, **AUX), ("fit", device_split))
    assert tok.doc_tok_off.tolist() == plan[0]
    # a call without fim= is the plain call again, and the flat calls never saw the stage
    plain, plain_off = F.flat(tokens)
    same(tok.encode_batch_padded(docs, layout="packed", device_split=device_split, **kw),
         mbpe.pack_tokens(plain, plain_off, layout="packed", **kw), "without fim")
    assert not tok.fim_info()[0].any()
    assert [t.tolist() for t in tok.encode_batch(docs, device_split=device_split)] == tokens


def test_decoding_gives_the_names_around_the_bytes(tok, case):
    docs, tokens, s, new, plan, spec = case
    got = tok.decode_batch(new)
    parts = [tok.decode_batch([t[:a], t[a:b], t[b:]]) for t, (a, b) in zip(tokens, plan[2])]
    for d, (text, out, mode, (P, M, S)) in enumerate(zip(docs, got, plan[1], parts)):
        if mode == F.NONE:
            assert out == text, d
            continue
        assert P + M + S == text, d
        if mode == F.PSM:
            assert out == NAMES["pre"] + P + NAMES["suf"] + S + NAMES["mid"] + M, d
        else:
            assert out == NAMES["pre"] + NAMES["suf"] + S + NAMES["mid"] + P + M, d
