"""Multi-turn conversations on the device: mbpe.turns_tokens -- ids, targets, offsets and info -- equals
tests/turns_cases.py (the rule in plain Python lists) on one mixed input that is the smallest at which each part of
csrc/turns.hip can go wrong, for both token widths, the three truncations and both label modes; then host and device
memory, an output off 16-byte alignment, the Encoder's stage through two layouts, its refusals, and the Tokenizer."""
import functools
import random

import numpy as np
import pytest

import mbpe
import oracle as O
import turns_cases as T
from conftest import read_data, read_golden
from test_gpu_textpair import from_device, on_device, same

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

TURN_END, END = 60001, 60002
MAX_TOKENS = (0, 1, 24)                  # none, the least, and one at which every mode bites on most conversations


@functools.lru_cache(maxsize=None)
def mixed(bits):
    """-> (turns as token lists, flat tokens, token offsets, turn_off, flags).  1,100 conversations of 0 .. 6 turns of
    0 .. 12 tokens (both scans cross a span of 1,024: 2,049+ turns), empty conversations and turns among them; one
    conversation of 300 one-token turns (more record boundaries than the 256-entry LDS table holds); one turn of 20,000
    tokens (it covers whole wave spans of 1,024 pieces)."""
    rng = random.Random(bits)
    convs = [[(rng.choice((0, 1, 1, 2, 5, 12)), rng.randrange(4)) for _ in range(rng.randrange(7))] for _ in range(1100)]
    convs[40] = [(1, rng.randrange(4)) for _ in range(300)]
    convs[700] = [(3, 0), (20000, 1), (2, 0), (4, 1)]
    convs[0], convs[1099] = [], []
    top = 60000 if bits == 16 else 1 << 31
    docs = [[rng.randrange(top) | (rng.randrange(2) << 31 if bits == 32 else 0) for _ in range(n)] for c in convs for n, _ in c]
    flags = np.array([f for c in convs for _, f in c], dtype=np.uint8)
    turn_off = np.concatenate([[0], np.cumsum([len(c) for c in convs])]).astype(np.uint64)
    assert len(docs) >= 2049
    flat = np.array([x for d in docs for x in d], dtype=np.uint16 if bits == 16 else np.uint32)
    off = np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.uint64)
    return docs, flat, off, turn_off, flags


@functools.lru_cache(maxsize=None)
def reference(bits, truncation, labels, K):
    """-> (spec keywords, the reference's ids, targets, offsets, info); head_turns 2 lies below and above the turn counts"""
    docs, _, _, turn_off, flags = mixed(bits)
    kw = dict(max_tokens=K, truncation=truncation, head_turns=2, turn_end_id=TURN_END, end_id=END, labels=labels)
    return (kw,) + T.join_all(docs, turn_off, flags, **kw)


@pytest.mark.parametrize("labels", T.LABELS)
@pytest.mark.parametrize("truncation", T.TRUNCATIONS)
@pytest.mark.parametrize("bits", [16, 32])
def test_turns_tokens_equals_the_reference(bits, truncation, labels):
    _, flat, off, turn_off, flags = mixed(bits)
    for K in MAX_TOKENS:
        kw, want_ids, want_tgt, want_off, want_info = reference(bits, truncation, labels, K)
        ids, tgt, new_off, info = mbpe.turns_tokens(flat, off, turn_off, flags, mbpe.turns_spec(**kw))
        assert ids.dtype == flat.dtype and new_off.tolist() == want_off and info.tolist() == want_info, K
        assert np.array_equal(ids, want_ids) and np.array_equal(tgt, want_tgt), K
        if K == 24:
            assert any(d for d, _ in want_info) == (truncation == "drop_oldest") and any(c for _, c in want_info)
    assert mbpe.turns_kernel_ms() > 0


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "one element off"])
@pytest.mark.parametrize("bits", [16, 32])
def test_device_memory_and_an_output_off_alignment(bits, shift):
    _, flat, off, turn_off, flags = mixed(bits)
    dtype = flat.dtype
    for truncation, K in (("drop_oldest", 0), ("left", 24)):
        kw, want_ids, want_tgt, want_off, want_info = reference(bits, truncation, "trained", K)
        n, s_ids, s_tgt = len(want_ids), shift * dtype.itemsize, shift * 4
        d_tok, p_tok = on_device(flat, 0)
        d_ids, p_ids = on_device(np.zeros(n, dtype=dtype), s_ids)
        d_tgt, p_tgt = on_device(np.zeros(n, dtype=np.uint32), s_tgt)
        torch.cuda.synchronize()
        got_n, new_off, info = mbpe.turns_tokens(None, off, turn_off, flags, mbpe.turns_spec(**kw), tokens_ptr=p_tok,
                                                 n_tokens=len(flat), token_bits=bits, out_ptr=p_ids, targets_ptr=p_tgt, cap=n)
        torch.cuda.synchronize()
        assert got_n == n and new_off.tolist() == want_off and info.tolist() == want_info
        assert np.array_equal(from_device(d_ids, s_ids, n, dtype), want_ids)
        assert np.array_equal(from_device(d_tgt, s_tgt, n, np.uint32), want_tgt)


# ---- through the Encoder and the Tokenizer ----------------------------------------------------------------------------------

SPEC = dict(max_tokens=60, truncation="drop_oldest", head_turns=1, turn_end_id=100258, end_id=100259, labels="trained")


def conversations():
    ts = read_data("taylorswift.txt")
    cut = lambda a, n: ts[a:a + n]
    return [[(cut(0, 40), False), (b"<|user|>\n", False, True), (cut(100, 70), False), (b"<|assistant|>\n", False, True),
             (cut(300, 90), True), (b"<|user|>\n", False, True), (cut(500, 30), False), (cut(700, 120), True)],
            [], [(b"", True)], [(cut(900, 400), False), (cut(1500, 25), True)], [(cut(1800, 5), False), (cut(2100, 60), True)]]


def joined(tokens, convs):
    turn_off = np.concatenate([[0], np.cumsum([len(c) for c in convs])])
    flags = [(T.TRAIN if t[1] else 0) | (T.NO_END if len(t) > 2 and t[2] else 0) for c in convs for t in c]
    flat, tgt, off, info = T.join_all(tokens, turn_off, flags, **SPEC)
    assert any(d for d, _ in info) and any(c for _, c in info)
    return np.array(flat, dtype=np.uint32), np.array(tgt, dtype=np.uint32), off, info, turn_off, flags


def test_encoder_stage_layouts_alloc_count_and_refusals():
    convs = conversations()
    texts = [t[0] for c in convs for t in c]
    merges = O.parse_model(read_golden("taylorswift_gpt4_first_512.model"))[2]
    kw = dict(seq_len=64, labels=True, segments=True)
    with mbpe.Encoder(merges) as enc:
        before = enc.encode_batch_aux(texts, seq_len=512, segments=True)
        tokens = [row[:n].tolist() for row, n in zip(before["ids"], before["lengths"])]
        flat, tgt, off, info, turn_off, flags = joined(tokens, convs)
        enc.set_turns(mbpe.turns_spec(**SPEC), turn_off, flags)
        same(enc.encode_batch_aux(texts, **kw), mbpe.pack_tokens_aux(flat, off, **kw, label_tokens=tgt), "aux")
        assert enc.doc_tok_off.tolist() == off and enc.turns_info().tolist() == info
        assert enc.n_tokens == sum(len(t) for t in tokens)       # "tokens encoded"
        fit = dict(doc_row=True, doc_col=True, cu_seqlens=True, **kw)
        same(enc.encode_batch_fit(texts, **fit), mbpe.pack_fit(flat, off, **fit, label_tokens=tgt), "fit")
        allocs = enc.alloc_count()
        enc.encode_batch_aux(texts, **kw)
        enc.encode_batch_fit(texts, **fit)
        assert enc.alloc_count() == allocs                       # a repeat call allocates nothing
        # never a silent choice: a wrong document count, another stage beside this one, the denoise calls
        def refused(call):
            with pytest.raises(mbpe.MbpeError) as e:
                call()
            assert e.value.code == mbpe.ERR_ARG
        refused(lambda: enc.encode_batch_aux(texts[:-1], **kw))
        refused(lambda: enc.encode_batch_denoise(texts, enc_len=64, dec_len=64, denoise=mbpe.denoise_spec(sentinel_id=100300)))
        for stage, spec in ((enc.set_fim, mbpe.fim_spec(1, 0.5, 100260, 100261, 100262)),
                            (enc.set_mlm, mbpe.mlm_spec(0.15, 100263, 768)), (enc.set_textpair, mbpe.textpair_spec())):
            stage(spec)
            refused(lambda: enc.encode_batch_aux(texts, **kw))
            stage(None)
        enc.set_turns(None)
        same(enc.encode_batch_aux(texts, seq_len=512, segments=True), before, "stage off")
        assert enc.alloc_count() == allocs and len(enc.turns_info()) == 0


def test_tokenizer_batch_aux_with_turns():
    pattern, _, merges = O.parse_model(read_golden("taylorswift_gpt4_first_512.model"))
    convs = conversations()
    tok = mbpe.Tokenizer(pattern)
    try:
        tok.set_special_tokens_from_file(read_data("special1.txt"))
        tok.set_merges(merges)
        tokens = [t.tolist() for t in tok.encode_batch([t[0] for c in convs for t in c])]
        flat, tgt, off, info, _, _ = joined(tokens, convs)
        kw = dict(seq_len=64, pad_id=0, eos_id=100257, labels=True, positions=True, segments=True)
        same(tok.encode_batch_aux(convs, **kw, turns=mbpe.turns_spec(**SPEC)),
             mbpe.pack_tokens_aux(flat, off, **kw, label_tokens=tgt), "tokenizer")
        assert tok.doc_tok_off.tolist() == off and tok.turns_info().tolist() == info
        texts = [t[0] for c in convs for t in c]                 # a call without turns= is the plain call again
        plain_off = np.concatenate([[0], np.cumsum([len(t) for t in tokens])])
        same(tok.encode_batch_aux(texts, **kw), mbpe.pack_tokens_aux(np.array([x for t in tokens for x in t], dtype=np.uint32),
                                                                     plain_off, **kw), "stage off")
        assert len(tok.turns_info()) == 0
    finally:
        tok.close()
