"""Span corruption on the GPU.  mbpe.denoise_tokens against denoise_cases.ref_apply, which builds both streams of every
unit from Python lists straight from the rule in include/mbpe.h: ids and offsets, exactly, for 16- and 32-bit tokens in
host and device memory, device outputs at every offset from 16-byte alignment, caps one too small.  The shapes are the
smallest at which each kernel can go wrong: the edges of the scans' spans of 1,024 in documents and in units, one
document of more than 1,024 units, runs of empty documents, one part and as many parts as there are sentinels, parts of
one token, a unit of 70,000 tokens in 35,000 parts, outputs of one id and of one 16-byte piece +- 1.  And the encoder's
calls: Encoder.encode_batch_denoise and encode_batch_endmask_denoise equal the composition "flat encode -> ref_apply ->
mbpe.pack_tokens / pack_tokens_aux" bit for bit."""
import ctypes
import random

import numpy as np
import pytest

import mbpe
import oracle as O
import denoise_cases as D
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
    return mbpe.DenoiseSpec(s["density"], s["seed"], s["doc_base"], s["mean_q8"], s["seg"], s["min_tokens"], s["sent"],
                            s["down"], s["n_sent"])


def want_of(docs, s, bits):
    """-> ((inputs, unit_in_off), (targets, unit_tg_off), unit_doc) of the reference."""
    ins, tgs, unit_doc = D.ref_apply(docs, s)
    return D.flat(ins, _TOK[bits]), D.flat(tgs, _TOK[bits]), unit_doc


def check(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    if not np.array_equal(got, want):
        at = int(np.flatnonzero(got != want)[0])
        raise AssertionError("%s: differs first at %d: got %d, want %d" % (what, at, got[at], want[at]))


def host_route(docs, s, bits, want, what):
    tokens, off = D.flat(docs, _TOK[bits])
    (w_in, w_ioff), (w_tg, w_toff), w_doc = want
    inp, tg, in_off, tg_off, unit_doc = mbpe.denoise_tokens(tokens, off, c_spec(s))
    assert in_off.tolist() == w_ioff.tolist() and tg_off.tolist() == w_toff.tolist(), what
    assert unit_doc.tolist() == w_doc, what
    check(inp, w_in, (what, "inputs"))
    check(tg, w_tg, (what, "targets"))


def device_route(dev, docs, s, bits, want, shift_in=1, shift_tg=1, flag_bit31=False, cap_in=None, cap_tg=None):
    """mbpe_denoise_tokens over device tokens into two device buffers that begin shift_in / shift_tg ids past a 16-byte
    boundary and have room for exactly the new ids, with guards on both sides -> (inputs, targets, guards ok, error)."""
    tb = bits // 8
    tokens, off = D.flat(docs, _TOK[bits])
    (w_in, w_ioff), (w_tg, w_toff), w_doc = want
    src = tokens
    if flag_bit31:                                               # as the encoder leaves them: bit 31 flags a chunk end
        rng = np.random.default_rng(7)
        src = tokens | (rng.integers(0, 2, len(tokens)).astype(np.uint32) << np.uint32(31))
    d_tok = torch.from_numpy(src.view({16: np.int16, 32: np.int32}[bits]).copy()).to(dev)
    bufs, ptrs = [], []
    for n, shift in ((len(w_in), shift_in), (len(w_tg), shift_tg)):
        b = torch.full((16 + shift * tb + n * tb + GUARD,), 0xAB, dtype=torch.uint8, device=dev)
        assert b.data_ptr() % 16 == 0
        bufs.append(b)
        ptrs.append(b.data_ptr() + 16 + shift * tb)
    torch.cuda.synchronize()
    err = None
    try:
        n_in, n_tg, in_off, tg_off, unit_doc = mbpe.denoise_tokens(
            None, off, c_spec(s), tokens_ptr=d_tok.data_ptr(), n_tokens=len(tokens), token_bits=bits, in_ptr=ptrs[0],
            cap_in=len(w_in) if cap_in is None else cap_in, tg_ptr=ptrs[1], cap_tg=len(w_tg) if cap_tg is None else cap_tg)
        assert (n_in, n_tg) == (len(w_in), len(w_tg))
        assert in_off.tolist() == w_ioff.tolist() and tg_off.tolist() == w_toff.tolist() and unit_doc.tolist() == w_doc
    except mbpe.MbpeError as e:
        err = e
    torch.cuda.synchronize()
    out, guards = [], True
    for b, n, shift in ((bufs[0], len(w_in), shift_in), (bufs[1], len(w_tg), shift_tg)):
        host = b.cpu().numpy()
        lo = 16 + shift * tb
        out.append(host[lo:lo + n * tb].view(_TOK[bits]).copy())
        guards = guards and bool((host[:lo] == 0xAB).all() and (host[lo + n * tb:] == 0xAB).all())
    return out[0], out[1], guards, err


def both_routes(dev, docs, s, bits, what, **kw):
    want = want_of(docs, s, bits)
    host_route(docs, s, bits, want, what)
    inp, tg, guards, err = device_route(dev, docs, s, bits, want, **kw)
    assert err is None and guards, what
    check(inp, want[0][0], (what, "device inputs"))
    check(tg, want[1][0], (what, "device targets"))
    return want


# ---- units and lengths ---------------------------------------------------------------------------------------------------

SEG = 7


@pytest.mark.parametrize("bits", [16, 32])
def test_small_documents_and_segment_edges(dev, bits):
    lens = [0, 1, 2, 3, SEG - 1, SEG, SEG + 1, 2 * SEG + 1, 0, 0, 5, 40, 0]
    docs = D.docs_of_lens(lens, random.Random(1))
    for s in (D.spec(D.threshold(0.5), 512, seed=2, seg=SEG), D.spec(D.threshold(0.5), 512, seed=2),
              D.spec(D.threshold(0.3), 768, seed=3, seg=SEG, min_tokens=4, down=0, sent=40000)):
        want = both_routes(dev, docs, s, bits, (bits, s), flag_bit31=bits == 32)
        if s["seg"]:
            n_units = [len(D.units_of(s, L)) for L in lens]
            assert n_units[:8] == [1, 1, 1, 1, 1, 1, 2, 3] and len(want[2]) == sum(n_units)
    assert mbpe.denoise_kernel_ms() > 0


def _edge_docs(kind, n, rng):
    if kind == "docs":                                           # n documents, a unit each
        lens = [rng.choice([0, 1, 2, 5, 9, 30]) for _ in range(n)]
    else:                                                        # n units: one document of 1,000, the rest one each
        lens = [SEG * 1000] + [rng.choice([0, 3, SEG]) for _ in range(n - 1000)]
    return D.docs_of_lens(lens, rng)


@pytest.mark.parametrize("kind", ["docs", "units"])
@pytest.mark.parametrize("n", [1023, 1024, 1025])
def test_scan_span_edges(dev, kind, n):
    docs = _edge_docs(kind, n, random.Random(n))
    s = D.spec(D.threshold(0.4), 512, seed=n, doc_base=1 << 40, seg=SEG if kind == "units" else 0)
    want = both_routes(dev, docs, s, 16, (kind, n))
    assert len(want[2]) == n


def test_one_document_of_more_than_1024_units_and_runs_of_empty_documents(dev):
    rng = random.Random(5)
    lens = [0] * 70 + [SEG * 1030 + 3] + [0] * 1100 + [4, 0, 0, 9] + [0] * 65
    docs = D.docs_of_lens(lens, rng)
    s = D.spec(D.threshold(0.5), 256, seed=5, seg=SEG)
    want = both_routes(dev, docs, s, 32, "long and empty")
    assert want[2].count(70) == 1031 and want[2].count(1174) == 2          # (the 9 tokens are two units too)
    assert len(want[2]) == 1031 + 2 + len(lens) - 2
    # all documents empty: units, and nothing to gather
    inp, tg, in_off, tg_off, unit_doc = mbpe.denoise_tokens(np.zeros(0, dtype=np.uint16), [0] * 6, c_spec(s))
    assert len(inp) == len(tg) == 0 and in_off.tolist() == tg_off.tolist() == [0] * 6 and unit_doc.tolist() == list(range(5))


# ---- the search for the part ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_sent", [1, 2, 3])
def test_as_many_parts_as_sentinels(dev, n_sent):
    lens = [2, 3, 4, 9, 33, 64, 65, 200]
    docs = D.docs_of_lens(lens, random.Random(n_sent))
    for down, sent in ((1, D.SENT), (0, 50000)):
        s = D.spec(D.threshold(0.5), 256, seed=n_sent, n_sent=n_sent, down=down, sent=sent)
        assert [D.counts(s, L)[1] for L in lens] == [min(L // 2, n_sent) for L in lens]
        for bits in (16, 32):
            want = both_routes(dev, docs, s, bits, (n_sent, down, bits), shift_in=3, shift_tg=2)
        last = sent - (n_sent - 1) if down else sent + n_sent - 1
        assert last in want[0][0] and last in want[1][0]


@pytest.mark.parametrize("density,mean_q8", [(1, 768), (D.ONE, 768), (D.ONE // 2, 256), (D.T5_DENSITY, 768)])
def test_densities_at_their_limits_and_parts_of_one(dev, density, mean_q8):
    lens = [0, 1, 2, 7, 8, 9, 100, 568, 1025]
    docs = D.docs_of_lens(lens, random.Random(9))
    s = D.spec(density, mean_q8, seed=4)
    cs = [D.counts(s, L) for L in lens]
    if density == 1:
        assert all(c == (1, 1) for c in cs[2:])                  # rounds to nothing: clamped to one token
    if density == D.ONE:
        assert all(c == (L - 1, 1) for c, L in zip(cs[2:], lens[2:]))    # all but one token, which stays the kept part
    if mean_q8 == 256:
        assert all(c == ((L + 1) // 2, min(L // 2, 100)) for c, L in zip(cs[2:], lens[2:]))
    for bits in (16, 32):
        both_routes(dev, docs, s, bits, (density, mean_q8, bits))


def test_anchors_on_the_device(dev):
    t5 = D.spec()
    for L, n_in, n_tg in ((568, 511, 113), (512, 461, 103)):
        inp, tg, in_off, tg_off, _ = mbpe.denoise_tokens(np.arange(L, dtype=np.uint16), [0, L], c_spec(t5))
        assert (len(inp), len(tg)) == (n_in, n_tg) and in_off.tolist() == [0, n_in] and tg_off.tolist() == [0, n_tg]
    inp, tg, _, _, _ = mbpe.denoise_tokens(np.arange(20, dtype=np.uint32), [0, 20], c_spec(t5))
    assert inp.tolist() == list(range(17)) + [32099] and tg.tolist() == [32099, 17, 18, 19]
    lens = [0, 1, 568, 1431]
    docs = [list(range(L)) for L in lens]
    want = both_routes(dev, docs, D.spec(seg=568), 16, "segments of 568")
    assert want[2] == [0, 1, 2, 3, 3, 3]


def test_search_depth_in_one_long_unit(dev):
    # 70,000 tokens, half of them noise, in 35,000 parts of one token: sixteen probes deep, every sentinel distinct
    docs = D.docs_of_lens([70000], random.Random(6), vocab=1000)
    s = D.spec(D.ONE // 2, 256, seed=6, n_sent=65000, down=0, sent=1000)
    assert D.counts(s, 70000) == (35000, 35000)
    both_routes(dev, docs, s, 32, "70,000 tokens", shift_in=2, shift_tg=3)
    s = D.spec(D.ONE // 2, 300, seed=6, n_sent=65000, down=1, sent=100000)
    assert D.counts(s, 70000)[1] == (35000 * 256 + 150) // 300
    both_routes(dev, docs, s, 32, "70,000 tokens, uneven strata")


# ---- pieces and widths ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits", [16, 32])
def test_every_offset_from_alignment(dev, bits):
    per = 128 // bits
    docs = D.docs_of_lens([5, 0, 12, 40, 3, 77], random.Random(4))
    s = D.spec(D.threshold(0.4), 512, seed=8)
    want = want_of(docs, s, bits)
    for k in range(per):                                         # inputs and targets move independently
        for shift_in, shift_tg in ((k, (3 * k + 1) % per), ((5 * k + 2) % per, k)):
            inp, tg, guards, err = device_route(dev, docs, s, bits, want, shift_in=shift_in, shift_tg=shift_tg,
                                                flag_bit31=bits == 32)
            assert err is None and guards, (shift_in, shift_tg)
            check(inp, want[0][0], (bits, shift_in, "inputs"))
            check(tg, want[1][0], (bits, shift_tg, "targets"))


@pytest.mark.parametrize("bits", [16, 32])
def test_totals_of_one_id_and_of_one_piece(dev, bits):
    per = 128 // bits
    seen_in, seen_tg = set(), set()
    rng = random.Random(3)
    s = D.spec(D.ONE // 2, 768, seed=2)
    for lens in [[1]] + [[L] for L in range(2, 2 * per + 8)] + [[0, L, 0] for L in (per - 1, per, per + 1)]:
        docs = D.docs_of_lens(lens, rng)
        sp = s if lens != [1] and len(lens) == 1 else dict(s, density=0)
        want = want_of(docs, sp, bits)
        seen_in.add(len(want[0][0]))
        seen_tg.add(len(want[1][0]))
        for shift in (0, 1, per - 1):
            inp, tg, guards, err = device_route(dev, docs, sp, bits, want, shift_in=shift, shift_tg=shift)
            assert err is None and guards, (lens, shift)
            check(inp, want[0][0], (bits, lens, shift, "inputs"))
            check(tg, want[1][0], (bits, lens, shift, "targets"))
    assert {1, per - 1, per, per + 1} <= seen_in and {per - 1, per, per + 1} <= seen_tg, (seen_in, seen_tg)


# ---- calls ---------------------------------------------------------------------------------------------------------------

def test_caps_too_small_write_nothing(dev):
    docs = D.docs_of_lens([5, 0, 12, 40], random.Random(4))
    s = D.spec(D.threshold(0.5), 512, seed=5)
    for bits in (16, 32):
        want = want_of(docs, s, bits)
        n_in, n_tg = len(want[0][0]), len(want[1][0])
        for kw in (dict(cap_in=n_in - 1), dict(cap_tg=n_tg - 1)):
            inp, tg, guards, err = device_route(dev, docs, s, bits, want, **kw)
            assert err is not None and err.code == mbpe.ERR_ARG and "too small" in str(err)
            assert guards and (inp.view(np.uint8) == 0xAB).all() and (tg.view(np.uint8) == 0xAB).all()
        # ... and the counts are still reported; host buffers stay as they were
        tokens, off = D.flat(docs, _TOK[bits])
        a, b = np.full(n_in, 0xABAB, dtype=_TOK[bits]), np.full(n_tg, 0xABAB, dtype=_TOK[bits])
        n = [ctypes.c_uint64(77) for _ in range(3)]
        rc = mbpe.lib().mbpe_denoise_tokens(0, tokens.ctypes.data, len(tokens), bits, 0, off.ctypes.data, len(off) - 1,
                                            ctypes.byref(c_spec(s)), a.ctypes.data, n_in, b.ctypes.data, n_tg - 1, 0, None,
                                            None, None, 0, *[ctypes.byref(x) for x in n])
        assert (rc, [x.value for x in n]) == (mbpe.ERR_ARG, [4, n_in, n_tg])
        assert (a == 0xABAB).all() and (b == 0xABAB).all()


def test_two_calls_with_doc_base_equal_one_and_a_repeat_is_identical(dev):
    rng = random.Random(8)
    docs = D.docs_of_lens([rng.randrange(0, 50) for _ in range(90)], rng)
    s = D.spec(D.threshold(0.3), 640, seed=31, doc_base=500, seg=16)
    tokens, off = D.flat(docs, np.uint16)
    whole = mbpe.denoise_tokens(tokens, off, c_spec(s))
    again = mbpe.denoise_tokens(tokens, off, c_spec(s))
    for a, b in zip(whole, again):
        assert np.array_equal(a, b)
    k = 37
    t1, o1 = D.flat(docs[:k], np.uint16)
    t2, o2 = D.flat(docs[k:], np.uint16)
    first = mbpe.denoise_tokens(t1, o1, c_spec(s))
    second = mbpe.denoise_tokens(t2, o2, c_spec(dict(s, doc_base=500 + k)))
    check(np.concatenate([first[0], second[0]]), whole[0], "inputs in two calls")
    check(np.concatenate([first[1], second[1]]), whole[1], "targets in two calls")
    assert first[4].tolist() + (second[4] + k).tolist() == whole[4].tolist()
    other = mbpe.denoise_tokens(tokens, off, c_spec(dict(s, seed=32)))
    assert not np.array_equal(other[0], whole[0]) and other[2].tolist() == whole[2].tolist()
    want = want_of(docs, s, 16)
    check(whole[0], want[0][0], "inputs")
    check(whole[1], want[1][0], "targets")


# ---- the encoder's calls -------------------------------------------------------------------------------------------------

MODEL = "taylorswift_gpt4_first_512"
PAD, START, EOS = 0, 700, 701
ENC_LEN, DEC_LEN = 24, 12
SENT0 = 699                                                      # 699, 698, ..: below the specials, above the merges


@pytest.fixture(scope="module")
def model():
    pattern, _, merges = O.parse_model(read_golden(MODEL + ".model"))
    return pattern, merges


def texts():
    """A dozen short texts, empty ones among them, and some longer than a segment and than a row."""
    ts = read_data("taylorswift.txt")
    out = [ts[a:a + n] for a, n in ((0, 40), (100, 7), (300, 90), (500, 1), (700, 60), (900, 25), (1200, 110), (1500, 33),
                                    (1800, 75), (2100, 12), (2400, 52))]
    out.insert(0, b"")
    out.insert(5, ts[9000:9400])
    out.append(b"")
    out.append(ts[20000:20700])
    out.append(b"")
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
    assert sorted(got) == sorted(want), (what, sorted(got), sorted(want))
    for k in want:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (what, k)


def composed(token_docs, s, out_bits, ignore):
    """The batch from the documents' tokens: the reference's two streams through the one-shot pack calls, rowwise."""
    ins, tgs, unit_doc = D.ref_apply(token_docs, s)
    dt = np.uint16 if out_bits == 16 else np.uint32
    fi, oi = D.flat(ins, dt)
    ft, ot = D.flat(tgs, dt)
    kw = dict(out_bits=out_bits, pad_id=PAD, eos_id=EOS)
    enc = mbpe.pack_tokens(fi, oi, ENC_LEN, **kw)
    dec = mbpe.pack_tokens_aux(ft, ot, DEC_LEN, bos_id=START, labels=True, ignore_label=ignore, **kw)
    return {"enc_ids": enc[0], "enc_len": enc[1], "dec_ids": dec["ids"], "dec_len": dec["lengths"],
            "dec_labels": dec["labels"], "row_doc": np.array(unit_doc, dtype=np.uint32)}


DSPEC = D.spec(D.threshold(0.3), 512, seed=17, doc_base=3, seg=30, sent=SENT0, n_sent=40)
BKW = dict(enc_len=ENC_LEN, dec_len=DEC_LEN, pad_id=PAD, eos_id=EOS, decoder_start_id=START)


@pytest.mark.parametrize("route", ["greedy", "dropout", "dedup"])
@pytest.mark.parametrize("out_bits,ignore", [(16, 65535), (32, -100), (64, -100)])
def test_encoder_calls_equal_the_composition(dev, model, route, out_bits, ignore):
    pattern, merges = model
    docs = texts()
    buf, off, doc_chunk = chunked(pattern, docs)
    doc_off = off[doc_chunk.astype(np.int64)]
    how = {"greedy": {}, "dropout": dict(rank_order=True, dropout=0.3, seed=5), "dedup": dict(dedup=True)}[route]
    kw = dict(BKW, out_bits=out_bits, ignore_label=ignore, denoise=c_spec(DSPEC))
    with mbpe.Splitter(pattern) as sp, mbpe.Encoder(merges, **how) as enc:
        sp.split_docs(buf, doc_off, [])
        mask_ptr, _, text_ptr = sp.endmask()
        tokens, chunk_tok = enc.encode(buf, off, offsets=True)
        doc_tok = chunk_tok[doc_chunk.astype(np.int64)].astype(np.int64)
        token_docs = [tokens[a:b].tolist() for a, b in zip(doc_tok[:-1], doc_tok[1:])]
        want = composed(token_docs, DSPEC, out_bits, ignore)
        n_rows = len(want["row_doc"])
        assert n_rows > len(docs) and max(len(t) for t in token_docs) > 3 * 30     # segments, and rows that truncate
        assert (want["enc_len"] == ENC_LEN).any() and (want["dec_len"] < DEC_LEN).any()

        def calls():
            a = enc.encode_batch_denoise(buf, off, doc_chunk, **kw)
            assert enc.n_tokens == len(tokens)
            b = enc.encode_batch_endmask_denoise(text_ptr, len(buf), mask_ptr, None, doc_off, **kw)
            assert enc.n_tokens == len(tokens)
            return a, b
        for got, name in zip(calls(), ("host split", "endmask")):
            same(got, want, (route, out_bits, name))
        assert enc.pack_ms() > 0 and enc.kernel_ms() >= enc.pack_ms()
        # the query: rows without matrices
        assert enc.encode_batch_denoise(buf, off, doc_chunk, **kw, ptrs={}) == n_rows and enc.n_rows == n_rows
        assert enc.encode_batch_endmask_denoise(text_ptr, len(buf), mask_ptr, None, doc_off, **kw, ptrs={}) == n_rows
        if route != "dedup":                                     # (the deduper's own buffers are its own matter)
            before = enc.alloc_count()
            for got, name in zip(calls(), ("host split", "endmask")):
                same(got, want, (route, out_bits, name, "repeat"))
            assert enc.alloc_count() == before
        # the plain batch calls are what they were
        plain = enc.encode_batch(buf, off, doc_chunk, seq_len=ENC_LEN, out_bits=out_bits)
        dt = np.uint16 if out_bits == 16 else np.uint32
        flat, foff = D.flat(token_docs, dt)
        for g, w in zip(plain, mbpe.pack_tokens(flat, foff, ENC_LEN, out_bits=out_bits)):
            assert np.array_equal(g, w)


def test_encoder_device_outputs_caps_and_refusals(dev, model):
    pattern, merges = model
    docs = texts()
    buf, off, doc_chunk = chunked(pattern, docs)
    kw = dict(BKW, denoise=c_spec(DSPEC))
    with mbpe.Encoder(merges) as enc:
        want = enc.encode_batch_denoise(buf, off, doc_chunk, **kw)
        n = len(want["row_doc"])
        shapes = dict(enc_ids=(n, ENC_LEN), enc_len=(n,), dec_ids=(n, DEC_LEN), dec_len=(n,), dec_labels=(n, DEC_LEN),
                      row_doc=(n,))
        t = {k: torch.full(sh, -1, dtype=torch.int32, device=dev) for k, sh in shapes.items()}
        torch.cuda.synchronize()
        ptrs = {k: v.data_ptr() for k, v in t.items()}
        with pytest.raises(mbpe.MbpeError) as e:                 # a cap too small writes nothing and reports the rows
            enc.encode_batch_denoise(buf, off, doc_chunk, **kw, ptrs=ptrs, cap_rows=n - 1)
        torch.cuda.synchronize()
        assert e.value.code == mbpe.ERR_ARG and "too small" in str(e.value) and enc.n_rows == n
        assert all(bool((v == -1).all()) for v in t.values())
        assert enc.encode_batch_denoise(buf, off, doc_chunk, **kw, ptrs=ptrs, cap_rows=n) == n
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy().view(np.int32 if k == "dec_labels" else np.uint32) for k, v in t.items()}
        same(got, want, "device outputs")
        # the matrices alone
        for v in t.values():
            v.fill_(-1)
        some = {k: ptrs[k] for k in ("enc_ids", "dec_ids")}
        assert enc.encode_batch_denoise(buf, off, doc_chunk, **kw, ptrs=some, cap_rows=n) == n
        torch.cuda.synchronize()
        assert np.array_equal(t["enc_ids"].cpu().numpy().view(np.uint32), want["enc_ids"])
        assert np.array_equal(t["dec_ids"].cpu().numpy().view(np.uint32), want["dec_ids"])
        assert bool((t["dec_labels"] == -1).all()) and bool((t["row_doc"] == -1).all())
        # never a silent choice: fill-in-the-middle or masked-LM on is the call's error
        enc.set_fim(mbpe.fim_spec(0.5, 0.5, 600, 601, 602))
        with pytest.raises(mbpe.MbpeError) as e:
            enc.encode_batch_denoise(buf, off, doc_chunk, **kw)
        assert e.value.code == mbpe.ERR_ARG
        enc.set_fim(None)
        enc.set_mlm(mbpe.mlm_spec(0.15, 600, 512))
        with pytest.raises(mbpe.MbpeError) as e:
            enc.encode_batch_denoise(buf, off, doc_chunk, **kw)
        assert e.value.code == mbpe.ERR_ARG
        enc.set_mlm(None)
        same(enc.encode_batch_denoise(buf, off, doc_chunk, **kw), want, "both off again")
        # a sentinel that does not fit a 16-bit matrix; specs that are not PADDED or differ in width
        big = c_spec(dict(DSPEC, sent=70000))
        with pytest.raises(mbpe.MbpeError) as e:
            enc.encode_batch_denoise(buf, off, doc_chunk, **dict(kw, denoise=big, out_bits=16, ignore_label=0))
        assert e.value.code == mbpe.ERR_VOCAB
        same(enc.encode_batch_denoise(buf, off, doc_chunk, **dict(kw, denoise=big)),
             composed_of(enc, buf, off, doc_chunk, dict(DSPEC, sent=70000)), "sentinels beyond 16 bits, 32-bit rows")
        L = mbpe.lib()
        es, ds = mbpe.pack_spec(ENC_LEN), mbpe.pack_spec(DEC_LEN)
        out = mbpe.DenoiseBatch(None, None, None, None, None, None, -100)
        text = np.frombuffer(buf, dtype=np.uint8)
        n_rows, n_tok = ctypes.c_uint64(77), ctypes.c_uint64(77)

        def raw(es, ds):
            return L.mbpe_encoder_encode_batch_denoise(enc._h, text.ctypes.data, len(text), 0, off.ctypes.data, len(off) - 1,
                                                       doc_chunk.ctypes.data, len(doc_chunk) - 1, ctypes.byref(c_spec(DSPEC)),
                                                       ctypes.byref(es), ctypes.byref(ds), ctypes.byref(out), 0, 0,
                                                       ctypes.byref(n_rows), ctypes.byref(n_tok))
        assert raw(es, ds) == mbpe.OK and n_rows.value == n
        assert raw(mbpe.pack_spec(ENC_LEN, "packed"), ds) == mbpe.ERR_ARG and n_rows.value == 0
        assert raw(es, mbpe.pack_spec(DEC_LEN, "packed")) == mbpe.ERR_ARG
        assert raw(es, mbpe.pack_spec(DEC_LEN, out_bits=64)) == mbpe.ERR_ARG


def composed_of(enc, buf, off, doc_chunk, s):
    tokens, chunk_tok = enc.encode(buf, off, offsets=True)
    doc_tok = chunk_tok[doc_chunk.astype(np.int64)].astype(np.int64)
    return composed([tokens[a:b].tolist() for a, b in zip(doc_tok[:-1], doc_tok[1:])], s, 32, -100)


def test_encoder_without_segments_and_without_documents(dev, model):
    pattern, merges = model
    docs = texts()
    buf, off, doc_chunk = chunked(pattern, docs)
    s = dict(DSPEC, seg=0, n_sent=3)
    kw = dict(BKW, denoise=c_spec(s))
    with mbpe.Encoder(merges) as enc:
        got = enc.encode_batch_denoise(buf, off, doc_chunk, **kw)
        same(got, composed_of(enc, buf, off, doc_chunk, s), "row i is document i")
        assert got["row_doc"].tolist() == list(range(len(docs)))
        # empty texts alone: rows of eos, and of the start id and eos
        got = enc.encode_batch_denoise([b"", b""], **kw)
        assert got["enc_len"].tolist() == [1, 1] and got["dec_len"].tolist() == [2, 2]
        assert got["enc_ids"][:, 0].tolist() == [EOS, EOS] and got["dec_ids"][:, :2].tolist() == [[START, EOS]] * 2
        assert got["dec_labels"][:, :2].tolist() == [[EOS, -100]] * 2
        got = enc.encode_batch_denoise([], **kw)
        assert got["enc_ids"].shape == (0, ENC_LEN) and got["dec_ids"].shape == (0, DEC_LEN)
