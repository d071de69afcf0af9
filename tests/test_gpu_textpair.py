"""Text pairs on the device: mbpe.textpair_tokens -- ids, targets, offsets and kept -- equals the reference of
tests/test_textpair_cpu.py (a literal statement of the rule) at the smallest shapes that can break the kernels, for both
token widths, host and device memory, the three truncations and both label modes; and Tokenizer.encode_batch_*(pairs,
textpair=spec) equals "encode each text alone -> reference join -> mbpe.pack_* with label_tokens"."""
import ctypes
import functools
import random

import numpy as np
import pytest

import mbpe
import oracle as O
from conftest import read_data, read_golden
from test_textpair_cpu import TRUNCATIONS, ref_join_all

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

SEP, SEP2, END = 60001, 60002, 60003
GUARD = 64
# empty sides, la == lb and one apart around K = 7 and 8, one side far longer
SMALL = [(0, 5), (5, 0), (0, 0), (4, 4), (4, 5), (5, 4), (7, 7), (1, 9), (9, 1), (3, 3), (8, 2), (0, 0), (2, 1)]
# (name, lens or (n_pairs, seed), keywords of textpair_spec): pairs and joined ids cross the spans of 1,024
CASES = [("small %d %s %d %s" % (len(sep), end, K, tail), SMALL,
          dict(sep_ids=sep, end_id=end, max_tokens=K + len(sep) + (end is not None), keep_tail_a=tail, keep_tail_b=tail))
         for sep, end in (((), None), ((SEP,), None), ((SEP, SEP2), END)) for K in (7, 8) for tail in (False, True)]
CASES += [
    ("1025 pairs", (1025, 1), dict(sep_ids=(SEP,), end_id=END, max_tokens=30, keep_tail_a=True)),
    ("2049 pairs", (2049, 2), dict(sep_ids=(SEP, SEP2), keep_tail_b=True)),
    ("2049 bare pairs", (2049, 3), dict(max_tokens=9)),
    ("one long pair", [(5000, 3000)], dict(sep_ids=(SEP,), end_id=END, max_tokens=4097, keep_tail_a=True)),
]
# bytes the device pointers (tokens, ids, targets) are off 16-byte alignment
SHIFTS = {16: [(0, 0, 0), (2, 4, 4), (4, 2, 0)], 32: [(0, 0, 0), (4, 0, 4), (0, 4, 0), (4, 4, 4)]}


@functools.lru_cache(maxsize=None)
def reference(name, bits, truncation, labels):
    """-> (tokens as the call gets them, offsets, spec keywords, the reference's ids, targets, offsets, kept)"""
    _, lens, kw = next(c for c in CASES if c[0] == name)
    rng = random.Random(name)
    if isinstance(lens, tuple):
        lens = [(rng.randrange(41), rng.randrange(41)) for _ in range(lens[0])]
    top = 60000 if bits == 16 else 1 << 31
    docs = [[rng.randrange(top) | (rng.randrange(2) << 31 if bits == 32 else 0) for _ in range(n)] for p in lens for n in p]
    kw = dict(kw, truncation=truncation, labels=labels)
    flat = np.array([x for d in docs for x in d], dtype=np.uint16 if bits == 16 else np.uint32)
    off = np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.uint64)
    return (flat, off, kw) + ref_join_all(docs, **kw)


def on_device(arr, shift):
    """A copy of arr in device memory `shift` bytes off 16-byte alignment, 0xAB around it -> (tensor, address)."""
    raw = np.full(shift + arr.nbytes + GUARD, 0xAB, dtype=np.uint8)
    raw[shift:shift + arr.nbytes] = arr.view(np.uint8)
    t = torch.from_numpy(raw).cuda()
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + shift


def from_device(t, shift, n, dtype):
    raw = t.cpu().numpy()
    assert (raw[:shift] == 0xAB).all() and (raw[shift + n * np.dtype(dtype).itemsize:] == 0xAB).all(), "wrote outside"
    return np.frombuffer(raw[shift:shift + n * np.dtype(dtype).itemsize].tobytes(), dtype=dtype)


@pytest.mark.parametrize("labels", ["all", "second"])
@pytest.mark.parametrize("truncation", TRUNCATIONS)
@pytest.mark.parametrize("memory", ["host", "device"])
@pytest.mark.parametrize("bits", [16, 32])
def test_textpair_tokens_equals_the_reference(bits, memory, truncation, labels):
    dtype = np.uint16 if bits == 16 else np.uint32
    for i, (name, _, _) in enumerate(CASES):
        flat, off, kw, want_ids, want_tgt, want_off, want_kept = reference(name, bits, truncation, labels)
        spec = mbpe.textpair_spec(**kw)
        if memory == "host":
            ids, tgt, new_off, kept = mbpe.textpair_tokens(flat, off, spec)
            shifts = []
        else:
            # the small cases take turns at the alignments, the others see all of them
            shifts = [SHIFTS[bits][i % len(SHIFTS[bits])]] if name.startswith("small") else SHIFTS[bits]
        for s_tok, s_ids, s_tgt in shifts:
            n = len(want_ids)
            d_tok, p_tok = on_device(flat, s_tok)
            d_ids, p_ids = on_device(np.zeros(n, dtype=dtype), s_ids)
            d_tgt, p_tgt = on_device(np.zeros(n, dtype=np.uint32), s_tgt)
            torch.cuda.synchronize()
            # a cap below the count: refused, the count still reported, nothing written to device memory
            count = ctypes.c_uint64()
            rc = mbpe.lib().mbpe_textpair_tokens(0, p_tok, len(flat), bits, 1, off.ctypes.data, len(off) - 1,
                                                 ctypes.byref(spec), p_ids, p_tgt, n - 1, 1, None, None, ctypes.byref(count))
            assert (rc, count.value) == (mbpe.ERR_ARG, n), name
            assert not from_device(d_ids, s_ids, n, dtype).any() and not from_device(d_tgt, s_tgt, n, np.uint32).any()
            got_n, new_off, kept = mbpe.textpair_tokens(None, off, spec, tokens_ptr=p_tok, n_tokens=len(flat),
                                                        token_bits=bits, out_ptr=p_ids, targets_ptr=p_tgt, cap=n)
            torch.cuda.synchronize()
            assert got_n == n, name
            ids, tgt = from_device(d_ids, s_ids, n, dtype), from_device(d_tgt, s_tgt, n, np.uint32)
            assert (d_tok.cpu().numpy()[s_tok:s_tok + flat.nbytes] == flat.view(np.uint8)).all()
            assert ids.tolist() == want_ids and tgt.tolist() == want_tgt, (name, s_tok, s_ids, s_tgt)
        assert ids.dtype == dtype and ids.tolist() == want_ids, name
        assert tgt.tolist() == want_tgt, name
        assert new_off.tolist() == want_off and kept.tolist() == want_kept, name
    assert mbpe.textpair_kernel_ms() > 0


# ---- through the Tokenizer ------------------------------------------------------------------------------------------------

SEQ_LEN, PAD, EOS = 48, 0, 100257
AUX = dict(labels=True, positions=True, segments=True)
KW = dict(seq_len=SEQ_LEN, pad_id=PAD, eos_id=EOS)


@pytest.fixture(scope="module")
def tok():
    pattern, _, merges = O.parse_model(read_golden("taylorswift_gpt4_first_512.model"))
    t = mbpe.Tokenizer(pattern)
    t.set_special_tokens_from_file(read_data("special1.txt"))
    t.set_merges(merges)
    yield t
    t.close()


@pytest.fixture(scope="module")
def case(tok):
    """Pairs of texts, the reference's join of their tokens, and the spec: computed once."""
    ts = read_data("taylorswift.txt")
    cut = lambda a, n: ts[a:a + n]
    pairs = [(cut(0, 40), cut(100, 70)), (b"", cut(300, 90)), (cut(500, 30), b""), (b"", b""), (cut(700, 400), cut(900, 25)),
             (cut(1200, 110), cut(1500, 133)), (cut(1800, 5), cut(2100, 300))]
    texts = [t for p in pairs for t in p]
    tokens = [t.tolist() for t in tok.encode_batch(texts)]
    kw = dict(max_tokens=60, truncation="longest_first", sep_ids=(100258,), end_id=100259, labels="second", keep_tail_a=True)
    flat, tgt, off, kept = ref_join_all(tokens, **kw)
    assert any(a < len(A) for (a, _), A in zip(kept, tokens[::2])) and any(b < len(B) for (_, b), B in zip(kept, tokens[1::2]))
    return pairs, tokens, np.array(flat, dtype=np.uint32), np.array(tgt, dtype=np.uint32), off, kept, mbpe.textpair_spec(**kw)


def same(got, want, what):
    assert sorted(got) == sorted(want), what
    for k in want:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (what, k)


LAYOUTS = {
    "aux": (lambda t: t.encode_batch_aux, mbpe.pack_tokens_aux, {}),
    "windows": (lambda t: t.encode_batch_windows, mbpe.pack_windows, dict(stride=8, row_doc=True)),
    "fit": (lambda t: t.encode_batch_fit, mbpe.pack_fit, dict(doc_row=True, doc_col=True, cu_seqlens=True)),
}


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_batch_calls_equal_the_reference_through_pack(tok, case, layout):
    pairs, tokens, flat, tgt, off, kept, spec = case
    method, pack, extra = LAYOUTS[layout]
    same(method(tok)(pairs, **KW, **AUX, **extra, textpair=spec), pack(flat, off, **KW, **AUX, **extra, label_tokens=tgt),
         layout)
    assert tok.doc_tok_off.tolist() == off and tok.textpair_info().tolist() == kept
    with pytest.raises(mbpe.MbpeError) as e:
        method(tok)(pairs, **KW, **extra, textpair=spec, fim=mbpe.fim_spec(1, 0.5, 100260, 100261, 100262))
    assert e.value.code == mbpe.ERR_ARG
    # a call without textpair= is the plain call again
    texts = [t for p in pairs for t in p]
    plain = np.array([x for t in tokens for x in t], dtype=np.uint32)
    plain_off = np.concatenate([[0], np.cumsum([len(t) for t in tokens])])
    same(method(tok)(texts, **KW, **AUX, **extra), pack(plain, plain_off, **KW, **AUX, **extra), "stage off")
    assert len(tok.textpair_info()) == 0


def test_encoder_stage_on_and_off(case):
    pairs, _, _, _, _, _, spec = case
    texts = [t for p in pairs for t in p]
    merges = O.parse_model(read_golden("taylorswift_gpt4_first_512.model"))[2]
    kw = dict(seq_len=512, labels=True, segments=True)
    sp = dict(max_tokens=60, truncation="longest_first", sep_ids=(100258,), end_id=100259, labels="second", keep_tail_a=True)
    with mbpe.Encoder(merges) as enc:
        # (every text one chunk here: other tokens than the Tokenizer's split gives, the same rule)
        before = enc.encode_batch_aux(texts, **kw)
        tokens = [row[:n].tolist() for row, n in zip(before["ids"], before["lengths"])]
        flat, tgt, off, kept = ref_join_all(tokens, **sp)
        enc.set_textpair(spec)
        joined = enc.encode_batch_aux(texts, **kw)
        same(joined, mbpe.pack_tokens_aux(np.array(flat, dtype=np.uint32), off, **kw,
                                          label_tokens=np.array(tgt, dtype=np.uint32)), "encoder")
        assert enc.doc_tok_off.tolist() == off and enc.textpair_info().tolist() == kept
        assert enc.n_tokens == sum(len(t) for t in tokens)       # "tokens encoded"
        # cu_seqlens and the fit layout's per-document outputs are those of the joined documents
        flat, tgt = np.array(flat, dtype=np.uint32), np.array(tgt, dtype=np.uint32)
        cu = dict(seq_len=64, labels=True, cu_seqlens=True)
        same(enc.encode_batch_aux(texts, layout="packed", **cu),
             mbpe.pack_tokens_aux(flat, off, layout="packed", **cu, label_tokens=tgt), "packed cu_seqlens")
        same(enc.encode_batch_fit(texts, doc_row=True, doc_col=True, **cu),
             mbpe.pack_fit(flat, off, doc_row=True, doc_col=True, **cu, label_tokens=tgt), "fit cu_seqlens")
        assert enc.doc_tok_off.tolist() == off
        ids, lengths = enc.encode_batch(texts, seq_len=512)      # the plain call: the joined ids alone
        assert np.array_equal(ids, joined["ids"]) and np.array_equal(lengths, joined["lengths"])
        with pytest.raises(mbpe.MbpeError) as e:
            enc.encode_batch_aux(texts[:-1], **kw)               # an odd document count
        assert e.value.code == mbpe.ERR_ARG
        allocs = enc.alloc_count()
        enc.encode_batch_aux(texts, **kw)
        assert enc.alloc_count() == allocs                       # a repeat call allocates nothing
        enc.set_textpair(None)
        same(enc.encode_batch_aux(texts, **kw), before, "stage off")
        assert enc.alloc_count() == allocs and len(enc.textpair_info()) == 0
