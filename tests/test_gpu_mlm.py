"""GPU tests of masked-LM batches: mbpe_mlm_tokens against the rule restated in Python (mlm_cases.ref_apply), bit for
bit in the new stream and in the targets, on the smallest shapes that can break the kernels (a span is 1,024 tokens, a
16-byte piece 4 tokens of 32 bits or 8 of 16); and the three packers with a target stream as labels, checked cell by
cell against labels derived from the same call's segments, positions, row_tok0 and the documents' offsets, while the same
calls without one still equal the references of the existing pack tests."""
import ctypes
import random

import numpy as np
import pytest
import torch

import mbpe
import mlm_cases as M
from fit_cases import ref_fit
from test_gpu_pack_aux import ref_aux
from test_gpu_pack_fit import as_arrays as fit_arrays
from test_gpu_pack_windows import as_arrays as win_arrays, same
from window_cases import ref_windows

pytestmark = pytest.mark.gpu

PAD, BOS, EOS = 3, 1, 2
CASES = M.gpu_cases()
AUX = dict(labels=True, positions=True, segments=True)


@pytest.fixture(scope="module")
def dev():
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def _c(s):
    """mlm_cases.spec -> mbpe.MlmSpec"""
    return mbpe.MlmSpec(s["select"], s["mask"], s["random"], s["seed"], s["doc_base"], s["mask_id"], s["vocab_n"],
                        s["whole_word"], len(s["protect"]), (ctypes.c_uint32 * 8)(*s["protect"]))


def _specs(ids):
    """token-level and whole-word, with two ids of the stream protected, at a rate that selects and spares words"""
    prot = tuple(sorted(set(ids[:2])))
    return [M.spec(M.threshold(0.4), seed=11, doc_base=(1 << 64) - 2, whole_word=ww, protect=prot) for ww in (0, 1)]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_mlm_tokens_equals_the_rule(dev, case):
    _, ids, ends, off = case
    tokens = M.flagged(ids, ends)
    for s in _specs(ids):
        want_out, want_tgt = M.ref_apply(s, ids, ends, off)
        out, tgt = mbpe.mlm_tokens(tokens, off, _c(s))
        assert out.dtype == np.uint32 and tgt.dtype == np.uint32
        assert out.tolist() == want_out and tgt.tolist() == want_tgt, (case[0], s["whole_word"])
        assert mbpe.mlm_kernel_ms() > 0
    # word_ends= is bit 31
    s = _specs(ids)[1]
    out, tgt = mbpe.mlm_tokens(np.array(ids, dtype=np.uint32), off, _c(s), word_ends=ends)
    assert (out.tolist(), tgt.tolist()) == M.ref_apply(s, ids, ends, off)


def test_the_cases_hold_what_they_are_for():
    by = {c[0]: c for c in CASES}
    _, ids, ends, off = by["long_word"]
    assert not any(ends[1024:2048]) and len(ids) > 2500          # a whole span without a word start
    s = M.spec(M.threshold(0.5), seed=2, whole_word=1)
    tgt = M.ref_apply(s, ids, ends, off)[1]
    assert len({t != M.NO_TOKEN for t in tgt[3:2503]}) == 1      # the word is a target as a whole, or not at all
    _, ids, ends, off = by["span_edges"]
    assert ends[1022] and ends[1023] and not any(ends[1000:1022]) and not any(ends[1024:1050])
    _, ids, ends, off = by["unflagged_ends"]
    assert any(not ends[int(o) - 1] for o in off[1:]) and any(int(o) % 4 for o in off)
    assert sum(1 for a, b in zip(by["empties"][3][:-1], by["empties"][3][1:]) if a == b) > 1000


def test_sixteen_bit_tokens_with_an_odd_count(dev):
    rng = random.Random(16)
    for n in (1, 7, 1031, 2049):
        ids, ends, off = M.stream(M.split_lens(n, rng, 1 + n // 50), rng, hi=60000)
        s = M.spec(M.threshold(0.4), seed=n, mask_id=65535, vocab_n=65536, protect=(ids[0],))
        out, tgt = mbpe.mlm_tokens(np.array(ids, dtype=np.uint16), off, _c(s))
        assert out.dtype == np.uint16 and tgt.dtype == np.uint32
        assert (out.tolist(), tgt.tolist()) == M.ref_apply(s, ids, ends, off)
    with pytest.raises(mbpe.MbpeError) as e:                     # 16-bit tokens carry no word ends
        mbpe.mlm_tokens(np.array(ids, dtype=np.uint16), off, _c(dict(s, whole_word=1)))
    assert e.value.code == mbpe.ERR_ARG


@pytest.mark.parametrize("shift", [0, 1])
def test_device_input_and_output_with_host_offsets(dev, shift):
    """shift 1: the three streams start 4 bytes behind a 16-byte boundary, so the kernels go id by id"""
    rng = random.Random(40 + shift)
    ids, ends, off = M.stream(M.split_lens(2500, rng, 30), rng)
    n = len(ids)
    GUARD = 16
    src = torch.zeros(n + shift + GUARD, dtype=torch.int32, device=dev)
    src[shift:shift + n] = torch.from_numpy(M.flagged(ids, ends).view(np.int32)).to(dev)
    for s in _specs(ids):
        want_out, want_tgt = M.ref_apply(s, ids, ends, off)
        out = torch.full((n + shift + GUARD,), -7, dtype=torch.int32, device=dev)
        tgt = torch.full((n + shift + GUARD,), -7, dtype=torch.int32, device=dev)
        assert mbpe.mlm_tokens(None, off, _c(s), tokens_ptr=src.data_ptr() + 4 * shift, n_tokens=n, token_bits=32,
                               out_ptr=out.data_ptr() + 4 * shift, targets_ptr=tgt.data_ptr() + 4 * shift) is None
        torch.cuda.synchronize()
        got_out, got_tgt = out.cpu().numpy().view(np.uint32), tgt.cpu().numpy().view(np.uint32)
        assert got_out[shift:shift + n].tolist() == want_out and got_tgt[shift:shift + n].tolist() == want_tgt
        for g in (got_out, got_tgt):                             # nothing before or behind the streams
            assert (g[:shift].view(np.int32) == -7).all() and (g[shift + n:].view(np.int32) == -7).all()
        # without targets
        out.fill_(-7)
        mbpe.mlm_tokens(None, off, _c(s), tokens_ptr=src.data_ptr() + 4 * shift, n_tokens=n, token_bits=32,
                        out_ptr=out.data_ptr() + 4 * shift, targets_ptr=None)
        torch.cuda.synchronize()
        assert out.cpu().numpy().view(np.uint32)[shift:shift + n].tolist() == want_out


def test_extremes(dev):
    rng = random.Random(8)
    ids, ends, off = M.stream(M.split_lens(1500, rng, 20), rng)
    tokens = M.flagged(ids, ends)
    for ww in (0, 1):
        out, tgt = mbpe.mlm_tokens(tokens, off, _c(M.spec(M.ONE, M.ONE, 0, whole_word=ww)))
        assert set(out.tolist()) == {M.MASK_ID} and tgt.tolist() == ids
        out, tgt = mbpe.mlm_tokens(tokens, off, _c(M.spec(0, whole_word=ww)))
        assert out.tolist() == ids and set(tgt.tolist()) == {M.NO_TOKEN}
        out, tgt = mbpe.mlm_tokens(tokens, off, _c(M.spec(M.ONE, 0, M.ONE, vocab_n=7, whole_word=ww)))
        assert set(out.tolist()) == set(range(7)) and tgt.tolist() == ids
    # one call of N documents equals two calls with doc_base
    s = M.spec(M.threshold(0.5), seed=3, doc_base=77, whole_word=1)
    whole = mbpe.mlm_tokens(tokens, off, _c(s))
    k, a = 9, int(off[9])
    part = mbpe.mlm_tokens(tokens[a:], off[k:] - off[k], _c(dict(s, doc_base=77 + k)))
    assert np.array_equal(part[0], whole[0][a:]) and np.array_equal(part[1], whole[1][a:])


# ---- the packers with a target stream -------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def masked(dev):
    """One masked stream for all packer tests: documents of 0 .. 40 tokens and two long ones -> (docs as lists of new
    ids, new ids, targets, offsets)."""
    rng = random.Random(77)
    lens = [0, 1, 2, 0, 5, 17, 40, 8, 9, 33, 0, 7, 16, 70, 3, 12, 130, 1]
    ids, ends, off = M.stream(lens, rng, hi=40000)
    s = M.spec(M.threshold(0.4), seed=5, whole_word=1, mask_id=40001, vocab_n=40000)
    out, tgt = mbpe.mlm_tokens(M.flagged(ids, ends), off, _c(s))
    assert (out.tolist(), tgt.tolist()) == M.ref_apply(s, ids, ends, off)
    docs = [out[int(a):int(b)].tolist() for a, b in zip(off[:-1], off[1:])]
    return docs, out, tgt, off


def _check_labels(got, plain, want_lab, what):
    """with label_tokens: everything but the labels is what the call gives without, and the labels are want_lab"""
    for k in plain:
        if k != "labels":
            assert np.array_equal(got[k], plain[k]), (what, k)
    assert got["labels"].dtype == plain["labels"].dtype
    if not np.array_equal(got["labels"].astype(np.int64), want_lab):
        at = tuple(np.argwhere(got["labels"].astype(np.int64) != want_lab)[0])
        raise AssertionError("%s: labels differ first at %s: got %s, want %s" % (what, at, got["labels"][at], want_lab[at]))


@pytest.mark.parametrize("layout,pad_left,trunc_left", [("padded", 0, 0), ("padded", 1, 0), ("padded", 0, 1), ("padded", 1, 1),
                                                        ("packed", 0, 0)])
def test_pack_tokens_aux_with_label_tokens(dev, masked, layout, pad_left, trunc_left):
    docs, out, tgt, off = masked
    L = np.diff(off).astype(np.int64)
    n_targets = 0
    for seq_len in (9, 16):
        for bos, eos in ((None, None), (BOS, EOS), (BOS, None)):
            nb, ne = int(bos is not None), int(eos is not None)
            keep = seq_len - nb - ne
            kw = dict(layout=layout, pad_id=PAD, bos_id=bos, eos_id=eos, pad_left=bool(pad_left), trunc_left=bool(trunc_left),
                      **AUX)
            what = (layout, pad_left, trunc_left, seq_len, bos, eos)
            plain = mbpe.pack_tokens_aux(out, off, seq_len, **kw)
            ref = ref_aux(out, off, seq_len, layout, 32, PAD, bos, eos, bool(pad_left), bool(trunc_left))
            for k, r in zip(("ids", "lengths", "labels", "positions", "segments"), ref):    # today's output
                assert np.array_equal(plain[k].astype(np.int64) & 0xFFFFFFFF, r.astype(np.int64)), (what, k)
            got = mbpe.pack_tokens_aux(out, off, seq_len, label_tokens=tgt, **kw)

            def tok_of(r, c, d, k):
                if layout == "packed":
                    return k - nb if nb <= k < nb + L[d] else None
                body = min(int(L[d]), keep)
                first = int(L[d]) - body if trunc_left else 0
                return first + k - nb if nb <= k < nb + body else None
            want = M.ref_labels(got, tgt, off, nb, ne, -100, tok_of)
            _check_labels(got, plain, want, what)
            n_targets += int((want != -100).sum())
    assert n_targets > 100


@pytest.mark.parametrize("score_once", [0, 1])
def test_pack_windows_with_label_tokens(dev, masked, score_once):
    docs, out, tgt, off = masked
    L = np.diff(off).astype(np.int64)
    for seq_len, stride in ((9, 0), (9, 3), (16, 5), (16, 13)):
        for bos, eos in ((None, None), (BOS, EOS)):
            nb, ne = int(bos is not None), int(eos is not None)
            if stride >= seq_len - nb - ne:
                continue
            keep = seq_len - nb - ne
            kw = dict(score_once=score_once, pad_id=PAD, bos_id=bos, eos_id=eos, row_doc=True, row_tok0=True, **AUX)
            what = (seq_len, stride, bos, eos, score_once)
            plain = mbpe.pack_windows(out, off, seq_len, stride, **kw)
            same(plain, win_arrays(ref_windows(docs, seq_len, stride, bos, eos, PAD, -100, score_once), seq_len, 32), what)
            got = mbpe.pack_windows(out, off, seq_len, stride, label_tokens=tgt, **kw)
            tok0 = got["row_tok0"]

            def tok_of(r, c, d, k):
                a = int(tok0[r])
                body = min(keep, int(L[d]) - a)
                if not nb <= k < nb + body:
                    return None
                if score_once and a > 0 and k < nb + stride:     # a cell the window before held too
                    return None
                return a + k - nb
            want = M.ref_labels(got, tgt, off, nb, ne, -100, tok_of)
            _check_labels(got, plain, want, what)
            if score_once:                                       # a token is a target at most once, and every target once
                seen = {}
                for r, c in np.argwhere(want != -100):
                    j = int(off[int(got["segments"][r, c]) - 1]) + int(tok0[r]) + int(got["positions"][r, c]) - nb
                    assert j not in seen
                    seen[j] = want[r, c]
                assert seen == {j: int(t) for j, t in enumerate(tgt.tolist()) if t != M.NO_TOKEN}


def test_pack_fit_with_label_tokens(dev, masked):
    docs, out, tgt, off = masked
    L = np.diff(off).astype(np.int64)
    for seq_len in (9, 16, 64):
        for bos, eos in ((None, None), (BOS, EOS), (None, EOS)):
            nb, ne = int(bos is not None), int(eos is not None)
            kw = dict(pad_id=PAD, bos_id=bos, eos_id=eos, doc_row=True, doc_col=True, **AUX)
            what = (seq_len, bos, eos)
            plain = mbpe.pack_fit(out, off, seq_len, **kw)
            same(plain, fit_arrays(ref_fit(docs, seq_len, bos, eos, PAD, -100), seq_len, 32), what)
            got = mbpe.pack_fit(out, off, seq_len, label_tokens=tgt, **kw)
            want = M.ref_labels(got, tgt, off, nb, ne, -100, lambda r, c, d, k: k - nb if nb <= k < nb + L[d] else None)
            _check_labels(got, plain, want, what)
            assert {int(t) for t in want[want != -100]} == {int(t) for t in tgt if t != M.NO_TOKEN}


def test_label_width_sixteen_and_device_target_stream(dev, masked):
    docs, out, tgt, off = masked
    out16 = out.astype(np.uint16)
    plain = mbpe.pack_tokens_aux(out16, off, 16, layout="packed", out_bits=16, pad_id=PAD, ignore_label=65535, **AUX)
    got = mbpe.pack_tokens_aux(out16, off, 16, layout="packed", out_bits=16, pad_id=PAD, ignore_label=65535, label_tokens=tgt,
                               **AUX)
    L = np.diff(off).astype(np.int64)
    want = M.ref_labels(got, tgt, off, 0, 0, 65535, lambda r, c, d, k: k if k < L[d] else None)
    _check_labels(got, plain, want, "16 bits")
    # tokens and the target stream in device memory, the matrices too
    n = len(out)
    d_tok = torch.from_numpy(out.view(np.int32)).to(dev)
    d_tgt = torch.from_numpy(tgt.view(np.int32)).to(dev)
    n_rows = (n + 15) // 16
    d_ids = torch.zeros(n_rows * 16 + 16, dtype=torch.int32, device=dev)
    d_lab = torch.zeros(n_rows * 16 + 16, dtype=torch.int32, device=dev)
    rows = mbpe.pack_tokens_aux(None, off, 16, layout="packed", pad_id=PAD, tokens_ptr=d_tok.data_ptr(), n_tokens=n,
                                token_bits=32, out_ptr=d_ids.data_ptr(), cap_rows=n_rows, labels_ptr=d_lab.data_ptr(),
                                label_tokens=d_tgt.data_ptr())
    torch.cuda.synchronize()
    assert rows == n_rows
    host = mbpe.pack_tokens_aux(out, off, 16, layout="packed", pad_id=PAD, labels=True, label_tokens=tgt)
    assert np.array_equal(d_ids.cpu().numpy()[:n_rows * 16].reshape(n_rows, 16).view(np.uint32), host["ids"])
    assert np.array_equal(d_lab.cpu().numpy()[:n_rows * 16].reshape(n_rows, 16), host["labels"])


def test_a_document_is_masked_alike_in_every_layout(dev, masked):
    """the mask belongs to the token in its document: (id, label) of every token is the same in all four layouts"""
    docs, out, tgt, off = masked
    L = np.diff(off).astype(np.int64)
    S = 140                                                       # no document is cut in "padded"
    layouts = {
        "padded": mbpe.pack_tokens_aux(out, off, S, layout="padded", pad_id=PAD, bos_id=BOS, label_tokens=tgt, **AUX),
        "packed": mbpe.pack_tokens_aux(out, off, 16, layout="packed", pad_id=PAD, bos_id=BOS, label_tokens=tgt, **AUX),
        "windows": mbpe.pack_windows(out, off, 16, 4, score_once=True, pad_id=PAD, bos_id=BOS, label_tokens=tgt,
                                     row_tok0=True, **AUX),
        "fit": mbpe.pack_fit(out, off, 16, pad_id=PAD, bos_id=BOS, label_tokens=tgt, **AUX),
    }
    want = {j: (int(out[j]), int(t) if t != M.NO_TOKEN else -100) for j, t in enumerate(tgt.tolist())}
    for name, m in layouts.items():
        seen = {}
        for r, c in np.argwhere(m["segments"] != 0):
            d, k = int(m["segments"][r, c]) - 1, int(m["positions"][r, c])
            a = int(m["row_tok0"][r]) if name == "windows" else 0
            if k < 1 or (name == "windows" and a > 0 and k < 1 + 4):
                continue                                         # bos, or a cell the window before held
            j = int(off[d]) + a + k - 1
            assert j not in seen, (name, j)
            seen[j] = (int(m["ids"][r, c]), int(m["labels"][r, c]))
        assert seen == want, name
