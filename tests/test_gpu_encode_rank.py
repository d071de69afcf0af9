"""Rank-ordered encode on the GPU: mbpe_encoder_set_option "rank_order", Tokenizer.encode(order="rank"), the command
line's --rank-order.

The judge is the pure-Python reference of tests/encode_rank_cases.py (the min-id loop over all chunks in numpy; the
CPU tests tie it to the literal loop and to the in-order replay).  Besides the tokens, every single-piece call is
held to the reference's passes: how many there were and how many tokens entered each (mbpe_encoder_pass_tokens) -- a
candidate that did not wait for its chunk's minimum, or one that waited for another chunk's, changes those counts even
where the final tokens come out the same.  The shapes are laid around groups of 64, spans of 1,024 and scan slices."""
import os
import subprocess

import numpy as np
import pytest

import mbpe
import oracle as O
import encode_cases as E
import encode_rank_cases as R
from conftest import DATA, ROOT, read_data, read_golden
from test_gpu_encode_split import Case as DeviceCase
from test_gpu_pack import ref_pack
from test_gpu_pack_aux import ref_aux

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CLI = os.path.join(ROOT, "minbpe-cc_amd", "minbpe-cc")
END = 0x80000000


@pytest.fixture(scope="module")
def dev():
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def _same(got, want, name):
    if len(got) != len(want) or not np.array_equal(got, want):
        n = min(len(got), len(want))
        diff = np.flatnonzero(np.asarray(got[:n]) != np.asarray(want[:n]))
        at = int(diff[0]) if len(diff) else n
        pytest.fail("%s: %d tokens, want %d; first difference at token %d: %s, want %s" % (
            name, len(got), len(want), at, got[max(at - 3, 0):at + 4].tolist(), want[max(at - 3, 0):at + 4].tolist()))


def _passes(pass_tokens, n_bytes):
    """The reference's pass_tokens as the device counts them: pass 1 sees every byte (the bytes of a chunk that is one
    token leave the stream in it, so a text with such a chunk and nothing to merge still takes two passes)."""
    if pass_tokens[0] == n_bytes:
        return pass_tokens
    return [n_bytes] + (pass_tokens[1:] if len(pass_tokens) > 1 else pass_tokens)


def _check(enc, c, ref=None):
    """One rank-ordered call against the reference: tokens, chunk offsets, passes and the tokens that entered each."""
    tok, end, pass_tokens = ref or R.reference(c)
    pass_tokens = _passes(pass_tokens, len(c.data))
    got, off = enc.encode(c.data, c.chunk_off, offsets=True)
    print(c.name, "passes", enc.n_passes, "want", len(pass_tokens))
    _same(got, tok, c.name)
    assert enc.n_passes == len(pass_tokens), (c.name, enc.n_passes, len(pass_tokens))
    assert enc.pass_tokens() == pass_tokens, (c.name, enc.pass_tokens(), pass_tokens)
    assert np.array_equal(off, R.chunk_tok_off(end, len(c.data), c.chunk_off)), c.name
    return got, off


def test_option_values():
    with mbpe.Encoder(R.PLACE_MERGES) as enc:
        for bad in (2, -1, 1 << 40):
            with pytest.raises(mbpe.MbpeError) as e:
                enc.set_option("rank_order", bad)
            assert e.value.code == mbpe.ERR_ARG
        # the three-byte witness: merges [(b,c), (a,b)], text abc
    with mbpe.Encoder(np.array([[98, 99], [97, 98]], dtype=np.uint32)) as enc:
        assert enc.encode(b"abc").tolist() == [257, 99]                      # the default: greedy
        enc.set_option("rank_order", 1)
        assert enc.encode(b"abc").tolist() == [97, 256]
    tok = mbpe.Tokenizer("")
    with pytest.raises(ValueError):
        tok.encode(b"abc", device=0, order="ranked")


def test_chunk_placement():
    c = R.placement_case()
    lens = np.diff(c.chunk_off.astype(np.int64))
    assert set(R.CHUNK_LENGTHS) <= set(lens.tolist())
    starts, ends = c.chunk_off[:-1].astype(np.int64), c.chunk_off[1:].astype(np.int64)
    for unit in (E.GROUP, E.SPAN):                              # the long chunks start and end on, before and behind edges
        for d in (-1, 0, 1):
            assert ((starts[lens > 60] - d) % unit == 0).any() and ((ends[lens > 60] - d) % unit == 0).any(), (unit, d)
    ref = R.reference(c)
    assert ref[2][1] < ref[2][0] and len(ref[2]) > 8
    with mbpe.Encoder(c.merges, rank_order=True) as enc:
        _check(enc, c, ref)
        # and the greedy order gives something else on this text
        enc.set_option("rank_order", 0)
        assert not np.array_equal(enc.encode(c.data, c.chunk_off), ref[0])


def test_runs_of_the_minimum_pair():
    cases = R.run_cases()
    assert len(cases) == 48
    with mbpe.Encoder(R.RUN_MERGES, rank_order=True) as enc:
        for c in cases:
            ref = R.reference(c)
            # with xy in the chunk the run waits: the first pass replaces exactly one pair
            assert (ref[2][0] - ref[2][1] == 1) == ("present" in c.name), c.name
            _check(enc, c, ref)


@pytest.mark.parametrize("index", range(3))
def test_one_chunk_over_the_scan_slices(index):
    c = R.slice_cases()[index]
    n_spans = -(-len(c.data) // E.SPAN)
    assert n_spans == 2 * E.SLICES + 1 and len(c.merges) <= 8
    ref = R.reference(c)
    assert len(ref[2]) <= 9
    if c.chunk_off is None:
        assert ref[2][0] - ref[2][1] == 1                            # pass 1: the one (a,b), everything else waits
    with mbpe.Encoder(c.merges, rank_order=True) as enc:
        _check(enc, c, ref)


def test_special_token_chunks(dev):
    c = R.special_case()
    ref = R.reference(c)
    assert sum(int(t) in R.SPECIAL_IDS for t in ref[0]) == 11
    with mbpe.Encoder(c.merges, rank_order=True) as enc:
        got, _ = _check(enc, c, ref)
        # the same positions as `singles` of the end-mask call; their bytes are ordinary text there
        s = R.special_case(as_singles=True)
        tok, end, pass_tokens = R.reference(s)
        d = DeviceCase(dev, s.data, s.chunk_off, np.arange(len(s.chunk_off)))
        got, doc_tok = enc.encode_endmask(*d.ptrs(), singles=s.singles, doc_off=d.doc_off)
        _same(got, tok, s.name)
        assert enc.n_passes == len(pass_tokens) and enc.pass_tokens() == _passes(pass_tokens, len(s.data))
        assert np.array_equal(doc_tok, R.chunk_tok_off(end, len(s.data), s.chunk_off))
        assert np.array_equal(tok, ref[0])                          # (the two texts differ in the markers' bytes only)


def test_pieces_and_formats(dev):
    c = R.fuzz_case(31, n_bytes=60000)
    tok, end, pass_tokens = R.reference(c)
    want_off = R.chunk_tok_off(end, len(c.data), c.chunk_off)
    with mbpe.Encoder(c.merges, rank_order=True) as enc:
        whole, _ = _check(enc, c, (tok, end, pass_tokens))
        enc.set_option("piece_bytes", 24000)
        off = [int(o) for o in c.chunk_off]
        cuts, c0 = 0, 0
        while c0 < len(off) - 1:                                     # the cut mbpe.h describes
            c1 = c0
            while c1 < len(off) - 1 and off[c1 + 1] - off[c0] <= 24000:
                c1 += 1
            cuts, c0 = cuts + 1, c1
        assert cuts == 3
        got, got_off = enc.encode(c.data, c.chunk_off, offsets=True)
        _same(got, tok, c.name + " in three pieces")
        assert np.array_equal(got_off, want_off)
        # 16-bit output, device text and output, the query, a cap that is too small: in pieces and whole
        for piece_bytes in (24000, 0):
            enc.set_option("piece_bytes", piece_bytes)
            assert np.array_equal(enc.encode(c.data, c.chunk_off, dtype=np.uint16), tok.astype(np.uint16))
            text = torch.from_numpy(np.ascontiguousarray(c.data).copy()).to(dev)
            out = torch.zeros(len(c.data), dtype=torch.int32, device=dev)
            n, off_dev = enc.encode_device(text.data_ptr(), len(c.data), c.chunk_off, out.data_ptr(), out.numel(),
                                           offsets=True)
            raw = out.cpu().numpy().view(np.uint32)
            assert n == len(tok) and np.array_equal(raw[:n] & np.uint32(END - 1), tok) and not raw[n:].any()
            assert np.array_equal((raw[:n] & np.uint32(END)) != 0, end) and np.array_equal(off_dev, want_off)
            assert enc.encode_device(text.data_ptr(), len(c.data), c.chunk_off, 0, 0) == len(tok)
            out.zero_()
            with pytest.raises(mbpe.MbpeError) as e:
                enc.encode_device(text.data_ptr(), len(c.data), c.chunk_off, out.data_ptr(), len(tok) - 1)
            assert e.value.code == mbpe.ERR_ARG and not out.cpu().numpy().any()


def test_batch_calls(dev):
    c = R.fuzz_case(31, n_bytes=60000)
    tok, end, _ = R.reference(c)
    chunk_tok = R.chunk_tok_off(end, len(c.data), c.chunk_off)
    n_chunks = len(c.chunk_off) - 1
    rng = np.random.default_rng(9)
    docs = np.unique(np.concatenate([[0, n_chunks], rng.integers(0, n_chunks, size=40)])).astype(np.uint64)
    doc_tok = chunk_tok[docs.astype(np.int64)]
    with mbpe.Encoder(c.merges, rank_order=True) as enc:
        for layout in ("padded", "packed"):
            kw = dict(seq_len=61, layout=layout, pad_id=3000, bos_id=None if layout == "packed" else 3001, eos_id=3002)
            ref_kw = dict(pad=3000, bos=kw["bos_id"], eos=3002)
            want_ids, want_len = ref_pack(tok, doc_tok, 61, layout, 32, **ref_kw)
            ids, lengths = enc.encode_batch(c.data, c.chunk_off, docs, **kw)
            assert np.array_equal(ids, want_ids) and np.array_equal(lengths, want_len), layout
            got = enc.encode_batch_aux(c.data, c.chunk_off, docs, labels=True, positions=True, segments=True, **kw)
            want = dict(zip(("ids", "lengths", "labels", "positions", "segments"),
                            ref_aux(tok, doc_tok, 61, layout, 32, **ref_kw)))
            assert np.array_equal(enc.doc_tok_off, doc_tok), layout
            for k in want:
                # (the labels come signed, the reference writes ignore_label truncated to the unsigned width)
                assert np.array_equal(np.asarray(got[k]).view(want[k].dtype), want[k]), (layout, k)
            # the end-mask form of the same chunks (no empty chunk in a mask: the fuzz cuts are distinct)
            d = DeviceCase(dev, c.data, c.chunk_off, docs)
            ids, lengths = enc.encode_batch_endmask(*d.ptrs(), None, d.doc_off, **kw)
            assert np.array_equal(ids, want_ids) and np.array_equal(lengths, want_len), layout
            assert np.array_equal(enc.doc_tok_off, doc_tok)


@pytest.mark.parametrize("seed", range(3))
def test_random_texts(seed):
    c = R.fuzz_case(100 + seed)
    assert R.well_formed(c.merges) and len(c.merges) <= 2000 - 256
    with mbpe.Encoder(c.merges, rank_order=True) as enc:
        _check(enc, c)


def test_one_encoder_both_orders():
    c = R.fuzz_case(33, n_bytes=100000)
    tok, _, pass_tokens = R.reference(c)
    greedy = O.encode_chunks(c.data, c.chunk_off, c.merges)
    assert not np.array_equal(greedy, tok)
    with mbpe.Encoder(c.merges) as enc:
        enc.set_option("rank_order", 1)
        _same(enc.encode(c.data, c.chunk_off), tok, "rank")
        a1 = enc.alloc_count()
        enc.set_option("rank_order", 0)
        _same(enc.encode(c.data, c.chunk_off), greedy, "greedy after rank")
        enc.set_option("rank_order", 1)
        _same(enc.encode(c.data, c.chunk_off), tok, "rank again")
        assert enc.n_passes == len(pass_tokens)
        assert enc.alloc_count() == a1                               # the repeat allocates nothing
    with mbpe.Encoder(c.merges) as enc:                              # the default allocates no rank buffers
        enc.encode(c.data, c.chunk_off)
        a0 = enc.alloc_count()
        enc.set_option("rank_order", 1)
        enc.encode(c.data, c.chunk_off)
        assert enc.alloc_count() == a0 + 2


@pytest.mark.parametrize("corpus", ["taylorswift gpt4", "splitmix one chunk"])
@pytest.mark.parametrize("mode", [1, 0])
def test_train_then_encode(corpus, mode):
    if corpus == "taylorswift gpt4":
        data = np.frombuffer(read_data("taylorswift.txt"), dtype=np.uint8)
        off = mbpe.presplit(O.GPT4_SPLIT_PATTERN, data)
    else:
        data, off = O.splitmix64_bytes(42, 1 << 16), None
    with mbpe.Trainer(0) as tr:
        merges = tr.train(data, 512, off, conflict_resolution=mode)[0]
        stream, ends = tr.stream()
    assert len(merges) == 256 and R.well_formed(merges)
    with mbpe.Encoder(merges, rank_order=True) as enc:
        got, tok_off = enc.encode(data, off, offsets=True)
        _same(got, stream, corpus + ": Encoder(rank_order) against Trainer.stream()")
        if off is None:                                              # (a corpus without chunks: the trainer flags no end)
            assert not ends.any() and tok_off.tolist() == [0, len(stream)]
        else:
            assert np.array_equal(np.flatnonzero(ends) + 1, np.unique(tok_off[1:]))
        enc.set_option("rank_order", 0)
        greedy = O.encode_chunks(data, off, merges)
        assert np.array_equal(enc.encode(data, off), greedy)
        # the greedy order is not the trainer's on text; on 64 KiB of random bytes no two of the 256 merges overlap
        # anywhere and the oracle's greedy encode equals the stream (both tie-breaks), so there is nothing to tell apart
        assert np.array_equal(greedy, stream) == (corpus == "splitmix one chunk")


def test_tokenizer_and_cli(tmp_path):
    tok = mbpe.Tokenizer(O.GPT4_SPLIT_PATTERN)
    tok.set_special_tokens_from_file(read_data("special1.txt"))
    tok.set_merges(O.parse_model(read_golden("taylorswift_gpt4_lexical_512.model"))[2])
    texts = [read_data("specialtokensample.txt"), b"", read_data("taylorswift.txt")[:20000], b"<|endoftext|>"]
    for t in texts:
        want = tok.encode(t, order="rank")                           # the host loop (tests/test_encode_rank_cpu.py)
        for split in (False, True, "unicode"):
            assert np.array_equal(tok.encode(t, device=0, device_split=split, order="rank"), want), split
    assert not np.array_equal(tok.encode(texts[2], device=0), tok.encode(texts[2], order="rank"))      # (per call)
    want = [tok.encode(t, order="rank") for t in texts]
    for split in (False, True):
        got = tok.encode_batch(texts, device_split=split, order="rank")
        assert [g.tolist() for g in got] == [w.tolist() for w in want]
        kw = dict(seq_len=48, layout="packed", pad_id=0, eos_id=100257)
        off = np.concatenate([[0], np.cumsum([len(w) for w in want])])
        want_ids, want_len = ref_pack(np.concatenate(want), off, 48, "packed", 32, pad=0, eos=100257)
        ids, lengths = tok.encode_batch_padded(texts, device_split=split, order="rank", **kw)
        assert np.array_equal(ids, want_ids) and np.array_equal(lengths, want_len)
        aux = tok.encode_batch_aux(texts, device_split=split, order="rank", labels=True, **kw)
        assert np.array_equal(aux["ids"], want_ids)
    # the command line: host, device, device with the device split -- byte for byte
    model = tmp_path / "m.model"
    tok.save(model)
    src = tmp_path / "in.txt"
    src.write_bytes(texts[0] + texts[2])
    outs = []
    for k, flags in enumerate((["--rank-order"], ["--rank-order", "--device-encode"],
                               ["--rank-order", "--device-encode", "--device-split"],
                               ["--rank-order", "--device-encode", "--device-split-unicode"], [])):
        out = tmp_path / ("enc%d" % k)
        r = subprocess.run([CLI, "--encode", "--input", str(src), "--model-path", str(model), "--output", str(out)] + flags,
                           capture_output=True, text=True)
        assert r.returncode == 0 and "Success" in r.stdout, r.stdout + r.stderr
        outs.append(out.read_bytes())
    assert outs[0] == outs[1] == outs[2] == outs[3] and len(outs[0]) > 0
    assert outs[0] == tok.encode(texts[0] + texts[2], order="rank").astype("<u4").tobytes()
    assert outs[4] != outs[0]                                        # without the flag: the greedy order
    tok.close()
