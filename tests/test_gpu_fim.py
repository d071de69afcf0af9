"""Fill-in-the-middle on the GPU.  mbpe.fim_tokens against fim_cases.ref_apply, which builds every document from
Python lists straight from the rule in include/mbpe.h: tokens and offsets, exactly, for 16- and 32-bit tokens in host
and device memory, an unaligned device output, one-too-small caps.  And the encoder's stage: with Encoder.set_fim every
batch call equals the composition "flat encode -> mbpe.fim_tokens -> mbpe.pack_*" bit for bit, and with the stage off
or its rate 0 it equals an encoder that never heard of it."""
import ctypes
import random

import numpy as np
import pytest

import mbpe
import oracle as O
import fim_cases as F
from conftest import read_data, read_golden

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

GUARD = 64
_TOK = {16: np.uint16, 32: np.uint32}


@pytest.fixture(scope="module")
def dev():
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def c_spec(s):
    return mbpe.FimSpec(s["rate"], s["spm"], s["seed"], s["doc_base"], s["pre"], s["suf"], s["mid"], s["min_tokens"],
                        s["max_tokens"])


def want_of(docs, s, bits):
    new = F.ref_apply(docs, s)
    tok, off = F.flat(new, _TOK[bits])
    return tok, off


def on_device(dev, tokens, off, s, bits, flag_bit31=False, cap=None):
    """mbpe_fim_tokens over device tokens into a device buffer that begins ONE TOKEN past a 16-byte boundary and has
    room for exactly the new tokens, with guards on both sides -> (tokens as numpy or None, count, offsets, guards ok)."""
    tb = bits // 8
    src = tokens
    if flag_bit31:                                               # as the encoder leaves them: bit 31 flags a chunk end
        src = tokens | np.where(np.arange(len(tokens)) % 3 == 0, np.uint32(1 << 31), np.uint32(0)).astype(np.uint32)
    d_tok = torch.from_numpy(src.view({16: np.int16, 32: np.int32}[bits]).copy()).to(dev)
    n_new = F.ref_plan([int(b - a) for a, b in zip(off[:-1], off[1:])], s)[0][-1]
    buf = torch.full((16 + n_new * tb + GUARD,), 0xAB, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    err = None
    try:
        n, new_off = mbpe.fim_tokens(None, off, c_spec(s), tokens_ptr=d_tok.data_ptr(), n_tokens=len(tokens),
                                     token_bits=bits, out_ptr=buf.data_ptr() + 16 + tb, cap=n_new if cap is None else cap)
    except mbpe.MbpeError as e:
        err, n, new_off = e, None, None
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    body = host[16 + tb:16 + tb + n_new * tb]
    guards = bool((host[:16 + tb] == 0xAB).all() and (host[16 + tb + n_new * tb:] == 0xAB).all())
    return body.view(_TOK[bits]).copy(), n, new_off, guards, err


def check(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    if not np.array_equal(got, want):
        at = int(np.flatnonzero(got != want)[0])
        raise AssertionError("%s: differs first at %d: got %d, want %d" % (what, at, got[at], want[at]))


@pytest.fixture(scope="module")
def mixed():
    """One batch whose cuts fall into different 16-byte pieces and spans, with its references for both widths."""
    rng = random.Random(1)
    docs = F.docs_of_lens(F.MIXED_LENS, rng)
    s = F.spec(F.ONE, F.threshold(0.5), seed=12)
    modes = F.ref_plan(F.MIXED_LENS, s)[1]
    assert F.PSM in modes and F.SPM in modes
    return docs, s, {bits: want_of(docs, s, bits) for bits in (16, 32)}


@pytest.mark.parametrize("bits", [16, 32])
def test_mixed_batch_host_and_device(dev, mixed, bits):
    docs, s, want = mixed
    want_tok, want_off = want[bits]
    tokens, off = F.flat(docs, _TOK[bits])
    got, new_off = mbpe.fim_tokens(tokens, off, c_spec(s))
    assert new_off.tolist() == want_off.tolist()
    check(got, want_tok, (bits, "host"))
    assert mbpe.fim_kernel_ms() > 0
    body, n, dev_off, guards, err = on_device(dev, tokens, off, s, bits, flag_bit31=bits == 32)
    assert err is None and n == len(want_tok) and dev_off.tolist() == want_off.tolist()
    check(body, want_tok, (bits, "device, one token past alignment"))
    assert guards
    # host tokens with bit 31 set are read without it
    if bits == 32:
        got, _ = mbpe.fim_tokens(tokens | np.uint32(1 << 31), off, c_spec(s))
        check(got, want_tok, "bit 31")


@pytest.mark.parametrize("bits", [16, 32])
def test_2049_documents(dev, bits):
    # the scan crosses two spans of 1,024 documents; rate 0.5 mixes copied and transformed documents
    lens = F.grid_lens(2049)
    docs = F.docs_of_lens(lens, random.Random(2))
    tokens, off = F.flat(docs, _TOK[bits])
    for s in (F.spec(F.threshold(0.5), F.threshold(0.5), seed=3, doc_base=1 << 40),
              F.spec(F.ONE, F.threshold(0.5), seed=4, min_tokens=5, max_tokens=30)):
        want_tok, want_off = want_of(docs, s, bits)
        got, new_off = mbpe.fim_tokens(tokens, off, c_spec(s))
        assert new_off.tolist() == want_off.tolist(), s
        check(got, want_tok, (bits, s))
        want_plan = F.ref_plan(lens, s)
        plan = mbpe.fim_plan(off, c_spec(s))
        assert plan[0].tolist() == want_plan[0] and plan[1].tolist() == want_plan[1] and plan[2].tolist() == want_plan[2]


@pytest.mark.parametrize("rate,spm", [(0.0, 0.0), (0.0, 1.0), (1.0, 0.0), (1.0, 1.0)])
def test_rates_zero_and_one(dev, rate, spm):
    lens = [0, 1, 9, 0, 0, 17, 2, 33]
    docs = F.docs_of_lens(lens, random.Random(3))
    s = F.spec(F.threshold(rate), F.threshold(spm), seed=8)
    modes = set(F.ref_plan(lens, s)[1])
    assert modes == ({F.NONE} if rate == 0 else {F.NONE, F.SPM if spm else F.PSM})   # (NONE: the empty documents)
    for bits in (16, 32):
        tokens, off = F.flat(docs, _TOK[bits])
        want_tok, want_off = want_of(docs, s, bits)
        got, new_off = mbpe.fim_tokens(tokens, off, c_spec(s))
        assert new_off.tolist() == want_off.tolist()
        check(got, want_tok, (bits, rate, spm, "host"))
        body, n, dev_off, guards, err = on_device(dev, tokens, off, s, bits)
        assert err is None and n == len(want_tok) and guards
        check(body, want_tok, (bits, rate, spm, "device"))


def test_cap_one_too_small_writes_nothing(dev):
    lens = [5, 0, 12, 40]
    docs = F.docs_of_lens(lens, random.Random(4))
    s = F.spec(F.ONE, F.threshold(0.5), seed=5)
    for bits in (16, 32):
        tokens, off = F.flat(docs, _TOK[bits])
        want_tok, want_off = want_of(docs, s, bits)
        body, n, dev_off, guards, err = on_device(dev, tokens, off, s, bits, cap=len(want_tok) - 1)
        assert err is not None and err.code == mbpe.ERR_ARG and "too small" in str(err)
        assert guards and (body.view(np.uint8) == 0xAB).all()
        # ... and the count is still reported
        n_out = ctypes.c_uint64(77)
        rc = mbpe.lib().mbpe_fim_tokens(0, tokens.ctypes.data, len(tokens), bits, 0, off.ctypes.data, len(off) - 1,
                                        ctypes.byref(c_spec(s)), body.ctypes.data, len(want_tok) - 1, 0, None,
                                        ctypes.byref(n_out))
        assert (rc, n_out.value) == (mbpe.ERR_ARG, len(want_tok))


# ---- the encoder's stage -------------------------------------------------------------------------------------------------

MODEL = "taylorswift_gpt4_first_512"
PRE, SUF, MID = 600, 601, 602
PAD, BOS, EOS = 0, 700, 701
SEQ_LEN = 48
AUX = dict(labels=True, positions=True, segments=True)


@pytest.fixture(scope="module")
def model():
    pattern, _, merges = O.parse_model(read_golden(MODEL + ".model"))
    return pattern, merges


def texts():
    """A dozen short texts, two empty ones among them, and two longer than a row."""
    ts = read_data("taylorswift.txt")
    out = [ts[a:a + n] for a, n in ((0, 40), (100, 7), (300, 90), (500, 1), (700, 60), (900, 25), (1200, 110), (1500, 33),
                                    (1800, 75), (2100, 12), (2400, 52))]
    out.insert(2, b"")
    out.insert(5, ts[9000:9400])
    out.append(b"")
    out.append(ts[20000:20700])
    return out


def chunked(pattern, docs):
    """The documents laid end to end, each split on its own -> (buffer, chunk_off, doc_chunk_off)."""
    off, doc_chunk, start = [0], [0], 0
    for d in docs:
        if d:
            off += (start + mbpe.presplit(pattern, np.frombuffer(d, dtype=np.uint8))[1:]).tolist()
        start += len(d)
        doc_chunk.append(len(off) - 1)
    return b"".join(docs), np.array(off, dtype=np.uint64), np.array(doc_chunk, dtype=np.uint64)


def same(got, want, what):
    if isinstance(want, tuple):
        got, want = dict(zip("ab", got)), dict(zip("ab", want))
    assert sorted(got) == sorted(want), what
    for k in want:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (what, k)


FSPEC = F.spec(F.threshold(0.75), F.threshold(0.5), seed=17, doc_base=3, pre=PRE, suf=SUF, mid=MID)


def batch_calls(enc, buf, off, doc_chunk, sp_ptrs, doc_off, out_bits, ignore):
    """Every batch call of the encoder, plain and _endmask -> {name: (result, doc_tok_off or None)}."""
    text_ptr, mask_ptr = sp_ptrs
    kw = dict(seq_len=SEQ_LEN, out_bits=out_bits, pad_id=PAD, bos_id=BOS, eos_id=EOS)
    akw = dict(kw, ignore_label=ignore, **AUX)
    out = {}

    def add(name, result, with_off=True):
        out[name] = (result, enc.doc_tok_off.copy() if with_off else None, enc.n_tokens)

    add("padded", enc.encode_batch(buf, off, doc_chunk, layout="padded", **kw), False)
    add("packed", enc.encode_batch(buf, off, doc_chunk, layout="packed", **kw), False)
    add("aux padded", enc.encode_batch_aux(buf, off, doc_chunk, layout="padded", cu_seqlens=False, **akw))
    add("aux packed", enc.encode_batch_aux(buf, off, doc_chunk, layout="packed", cu_seqlens=True, **akw))
    add("windows", enc.encode_batch_windows(buf, off, doc_chunk, stride=8, row_doc=True, row_tok0=True, **akw))
    add("fit", enc.encode_batch_fit(buf, off, doc_chunk, cu_seqlens=True, doc_row=True, doc_col=True, **akw))
    n = len(buf)
    add("endmask padded", enc.encode_batch_endmask(text_ptr, n, mask_ptr, None, doc_off, layout="padded", **kw))
    add("endmask packed", enc.encode_batch_endmask(text_ptr, n, mask_ptr, None, doc_off, layout="packed", **kw))
    add("endmask aux packed", enc.encode_batch_endmask(text_ptr, n, mask_ptr, None, doc_off, layout="packed",
                                                       cu_seqlens=True, **akw))
    add("endmask windows", enc.encode_batch_endmask_windows(text_ptr, n, mask_ptr, None, doc_off, stride=8, row_doc=True,
                                                            row_tok0=True, **akw))
    add("endmask fit", enc.encode_batch_endmask_fit(text_ptr, n, mask_ptr, None, doc_off, cu_seqlens=True, doc_row=True,
                                                    doc_col=True, **akw))
    return out


def composed(tokens, doc_tok, out_bits, ignore):
    """The same matrices from flat tokens through the one-shot pack calls."""
    kw = dict(seq_len=SEQ_LEN, out_bits=out_bits, pad_id=PAD, bos_id=BOS, eos_id=EOS)
    akw = dict(kw, ignore_label=ignore, **AUX)
    w = {
        "padded": mbpe.pack_tokens(tokens, doc_tok, layout="padded", **kw),
        "packed": mbpe.pack_tokens(tokens, doc_tok, layout="packed", **kw),
        "aux padded": mbpe.pack_tokens_aux(tokens, doc_tok, layout="padded", **akw),
        "aux packed": mbpe.pack_tokens_aux(tokens, doc_tok, layout="packed", cu_seqlens=True, **akw),
        "windows": mbpe.pack_windows(tokens, doc_tok, stride=8, row_doc=True, row_tok0=True, **akw),
        "fit": mbpe.pack_fit(tokens, doc_tok, cu_seqlens=True, doc_row=True, doc_col=True, **akw),
    }
    for k in ("padded", "packed", "aux packed", "windows", "fit"):
        w["endmask " + k] = w[k]
    return w


@pytest.mark.parametrize("route", ["greedy", "dropout", "dedup"])
@pytest.mark.parametrize("out_bits,ignore", [(16, 65535), (32, -100), (64, -100)])
def test_encoder_calls_equal_the_composition(dev, model, route, out_bits, ignore):
    pattern, merges = model
    docs = texts()
    buf, off, doc_chunk = chunked(pattern, docs)
    doc_off = off[doc_chunk.astype(np.int64)]
    how = {"greedy": {}, "dropout": dict(rank_order=True, dropout=0.3, seed=5), "dedup": dict(dedup=True)}[route]
    with mbpe.Splitter(pattern) as sp, mbpe.Encoder(merges, **how) as enc:
        sp.split_docs(buf, doc_off, [])
        mask_ptr, _, text_ptr = sp.endmask()
        enc.set_fim(c_spec(FSPEC))
        # the flat encode is unaffected by the stage
        tokens, chunk_tok = enc.encode(buf, off, dtype=np.uint16 if out_bits == 16 else np.uint32, offsets=True)
        doc_tok = chunk_tok[doc_chunk.astype(np.int64)]
        lens = np.diff(doc_tok.astype(np.int64)).tolist()
        assert PRE not in tokens.tolist() and len(tokens) == int(doc_tok[-1])
        ft, foff = mbpe.fim_tokens(tokens, doc_tok, c_spec(FSPEC))
        want_off, want_mode, want_cut = F.ref_plan(lens, FSPEC)
        assert foff.tolist() == want_off and {F.NONE, F.PSM, F.SPM} <= set(want_mode)
        n_done = sum(m != F.NONE for m in want_mode)
        want = composed(ft, foff, out_bits, ignore)
        got = batch_calls(enc, buf, off, doc_chunk, (text_ptr, mask_ptr), doc_off, out_bits, ignore)
        assert sorted(got) == sorted(want)
        for name, (result, tok_off, n_tokens) in got.items():
            same(result, want[name], (route, out_bits, name))
            # doc_tok_off_out: the offsets after the stage; n_tokens_out: the tokens encoded
            assert tok_off is None or tok_off.tolist() == want_off, name
            assert n_tokens == len(tokens) and want_off[-1] == n_tokens + 3 * n_done, name
        mode, cuts = enc.fim_info()
        assert mode.tolist() == want_mode and cuts.tolist() == want_cut
        assert enc.pack_ms() > 0 and enc.kernel_ms() >= enc.pack_ms()
        # a repeat call of no larger size allocates nothing
        if route != "dedup":                                     # (the deduper's own buffers are its own matter)
            before = enc.alloc_count()
            again = batch_calls(enc, buf, off, doc_chunk, (text_ptr, mask_ptr), doc_off, out_bits, ignore)
            for name in want:
                same(again[name][0], want[name], (route, out_bits, name, "repeat"))
            assert enc.alloc_count() == before


def test_encoder_device_outputs(dev, model):
    pattern, merges = model
    docs = texts()
    buf, off, doc_chunk = chunked(pattern, docs)
    kw = dict(seq_len=SEQ_LEN, pad_id=PAD, eos_id=EOS)
    with mbpe.Encoder(merges) as enc:
        enc.set_fim(c_spec(FSPEC))
        want = enc.encode_batch_fit(buf, off, doc_chunk, **kw, **AUX)
        tokens, chunk_tok = enc.encode(buf, off, offsets=True)
        ft, foff = mbpe.fim_tokens(tokens, chunk_tok[doc_chunk.astype(np.int64)], c_spec(FSPEC))
        same(want, mbpe.pack_fit(ft, foff, **kw, **AUX), "host")
        n = len(want["lengths"])
        d_ids, d_lab, d_pos = (torch.full((n, SEQ_LEN), -1, dtype=torch.int32, device=dev) for _ in range(3))
        d_len = torch.full((n,), -1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        rows = enc.encode_batch_fit(buf, off, doc_chunk, **kw, out_ptr=d_ids.data_ptr(), len_ptr=d_len.data_ptr(),
                                    cap_rows=n, labels_ptr=d_lab.data_ptr(), pos_ptr=d_pos.data_ptr())
        torch.cuda.synchronize()
        assert rows == n and enc.doc_tok_off.tolist() == foff.tolist()
        same({"ids": d_ids.cpu().numpy().view(np.uint32), "labels": d_lab.cpu().numpy(),
              "positions": d_pos.cpu().numpy().view(np.uint32), "lengths": d_len.cpu().numpy().view(np.uint32)},
             {k: want[k] for k in ("ids", "labels", "positions", "lengths")}, "device outputs")
        # PACKED rows into device memory
        ids, lengths = mbpe.pack_tokens(ft, foff, layout="packed", **kw)
        d_ids = torch.full(ids.shape, -1, dtype=torch.int32, device=dev)
        d_len = torch.full(lengths.shape, -1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        rows = enc.encode_batch(buf, off, doc_chunk, layout="packed", **kw, out_ptr=d_ids.data_ptr(),
                                len_ptr=d_len.data_ptr(), cap_rows=len(ids))
        torch.cuda.synchronize()
        assert rows == len(ids)
        same({"ids": d_ids.cpu().numpy().view(np.uint32), "lengths": d_len.cpu().numpy().view(np.uint32)},
             {"ids": ids, "lengths": lengths}, "packed, device")
        # a sentinel that does not fit a 16-bit matrix is refused by the call, before any work
        enc.set_fim(c_spec(dict(FSPEC, mid=70000)))
        with pytest.raises(mbpe.MbpeError) as e:
            enc.encode_batch(buf, off, doc_chunk, layout="packed", out_bits=16, seq_len=SEQ_LEN)
        assert e.value.code == mbpe.ERR_VOCAB


def test_stage_off_and_rate_zero_are_a_fresh_encoder(dev, model):
    pattern, merges = model
    docs = texts()
    buf, off, doc_chunk = chunked(pattern, docs)
    doc_off = off[doc_chunk.astype(np.int64)]
    with mbpe.Splitter(pattern) as sp:
        sp.split_docs(buf, doc_off, [])
        mask_ptr, _, text_ptr = sp.endmask()
        with mbpe.Encoder(merges) as fresh:
            want = batch_calls(fresh, buf, off, doc_chunk, (text_ptr, mask_ptr), doc_off, 32, -100)
            want_allocs = fresh.alloc_count()
            mode, cuts = fresh.fim_info()
            assert mode.tolist() == [0] * len(docs) and not cuts.any()
        for how in ("rate 0", "off again"):
            with mbpe.Encoder(merges) as enc:
                if how == "rate 0":
                    enc.set_fim(c_spec(dict(FSPEC, rate=0)))
                else:
                    enc.set_fim(c_spec(FSPEC))
                    enc.set_fim(None)
                got = batch_calls(enc, buf, off, doc_chunk, (text_ptr, mask_ptr), doc_off, 32, -100)
                for name, (result, tok_off, n_tokens) in want.items():
                    same(got[name][0], result, (how, name))
                    assert n_tokens == got[name][2] and (tok_off is None or tok_off.tolist() == got[name][1].tolist())
                assert enc.alloc_count() == want_allocs, how       # not one buffer more
                mode, cuts = enc.fim_info()
                assert mode.tolist() == [0] * len(docs) and not cuts.any()
        # turned off after it ran: the same matrices again
        with mbpe.Encoder(merges) as enc:
            enc.set_fim(c_spec(FSPEC))
            on = enc.encode_batch(buf, off, doc_chunk, layout="packed", seq_len=SEQ_LEN)
            assert on[0].tobytes() != want["packed"][0][0].tobytes() and enc.fim_info()[0].any()
            enc.set_fim(None)
            got = batch_calls(enc, buf, off, doc_chunk, (text_ptr, mask_ptr), doc_off, 32, -100)
            for name, (result, tok_off, n_tokens) in want.items():
                same(got[name][0], result, ("off after on", name))
            assert not enc.fim_info()[0].any()
