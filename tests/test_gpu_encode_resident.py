"""The encoder's option "resident" on the GPU: tokens, chunk token offsets and token byte offsets equal the per-chunk
Python loops of the case modules (greedy: byteoff_cases.encode_chunks; rank order and dropout: dropout_cases.reference)
at the shapes where the tiles' geometry (B = 768, L = 256) can go wrong."""
import numpy as np
import pytest

import mbpe
import oracle as O
import byteoff_cases as G
import dropout_cases as D
import encode_rank_cases as R
from conftest import read_data, read_golden
from test_gpu_encode_split import Case as DeviceCase

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

B, L = 768, 256
MODES = [("greedy", 0.0), ("rank", 0.0), ("rank", 0.3)]
SEED = 5
each_mode = pytest.mark.parametrize("mode", MODES, ids=lambda m: "%s-p%g" % m)
RUN_MERGES = np.array([(97, 97), (256, 256), (257, 257), (98, 99)], dtype=np.uint32)


def _reference(mode, data, off, merges):
    """-> (tokens, chunk token offsets, token byte offsets) by the per-chunk loops"""
    order, p = mode
    n = len(data)
    if order == "greedy":
        tok, boff = G.encode_chunks(data, off, merges.tolist())
        edges = [0, n] if off is None else off
        return tok, np.searchsorted(boff[:-1], edges).astype(np.uint64), boff
    tok, end, pos, _ = D.reference(data, off, merges, SEED, D.threshold_of(p))
    return tok, R.chunk_tok_off(end, n, off), D.byte_offsets(pos, n)


def _encoder(mode, merges, **kw):
    return mbpe.Encoder(merges, rank_order=mode[0] == "rank", dropout=mode[1], seed=SEED, resident=True, **kw)


def _check(enc, mode, name, data, off, merges, raw=None, boff=True, dtype=np.uint32):
    tok, tok_off, byte_off = _reference(mode, data, off, merges)
    got = enc.encode(data, off, offsets=True, byte_off=boff, dtype=dtype)
    assert np.array_equal(got[0], tok.astype(dtype)), name
    assert np.array_equal(got[1], tok_off), name
    if boff:
        assert np.array_equal(got[2], byte_off), name
    if not len(data):
        return
    st = enc.resident_stats()
    assert st["tiles"] >= -(-len(data) // B) and enc.pass_tokens()[0] == len(data), name
    assert raw is None or (st["raw_tiles"] > 0) == raw, (name, st)
    if st["raw_tiles"] == 0:
        assert enc.n_passes == 1 and st["tokens_after_stage"] == len(tok), (name, st)
    else:
        assert enc.n_passes >= 2 and st["tokens_after_stage"] > len(tok), (name, st)   # the raw tiles' merges are left


def _text(lens, seed=1, fill=None):
    """chunks of the given lengths over a, b, c, d (fill: {chunk index: bytes}) -> (data, chunk_off)"""
    rng = np.random.default_rng(seed)
    data = rng.choice(np.arange(97, 101, dtype=np.uint8), size=int(sum(lens)))
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    for c, b in (fill or {}).items():
        data[int(off[c]):int(off[c + 1])] = np.frombuffer(b, dtype=np.uint8)
    return data.tobytes(), off


def _around(first, last, total=3000, short=5):
    """short chunks, one chunk [first, last], one of 300 bytes behind it, short chunks up to `total`"""
    lens = [short] * (first // short) + ([first % short] if first % short else []) + [last - first + 1, 300]
    rest = total - sum(lens)
    return lens + [short] * (rest // short) + ([rest % short] if rest % short else [])


def _geometry_shapes():
    shapes = []
    for t in (1, 2):
        # the end bit at the first and last byte the search sees, and one beyond: beyond it the boundary is open
        for d in (-2, -1, 0, L - 3, L - 2, L - 1):
            e = t * B + d
            shapes.append(("end bit at %d B %+d" % (t, d), _text(_around(min(e - 40, t * B - 2), e)), not -1 <= d <= L - 2))
    for n in (255, 256, 257):                                     # a chunk around the search bound, from byte B - 1 on
        shapes.append(("chunk of %d bytes across B" % n, _text(_around(B - 1, B - 2 + n)), n > L))
    shapes.append(("tile of 1,023 tokens", _text(_around(700, B + L - 2)), False))
    shapes.append(("one chunk of 3,000 bytes", _text([7] * 150 + [3000] + [7] * 150), True))
    shapes.append(("short chunks", _text([9] * 400), False))
    shapes.append(("one-byte chunks", _text([1] * 2000), False))
    shapes.append(("empty text", (b"", None), None))
    shapes.append(("one byte", (b"c", None), False))
    for last in (B - 1, B):                                       # a one-token chunk whose bytes end at the boundary
        lens = _around(last - 5, last)
        shapes.append(("single that ends at byte %d" % last,
                       _text(lens, fill={lens.index(6): b"\x00  300", 3: b"\x00  7 "}), None))
    return shapes


@each_mode
def test_tile_geometry(mode):
    # 200 a's: (a,a) -> X, (X,X) -> Y, (Y,Y) -> Z; the run's parity crosses three groups of 64 lanes, round after round
    runs = [("run at chunk %d" % at, _text([5] * at + [200] + [5] * 300, fill={at: b"a" * 200}), False) for at in (0, 30, 61)]
    for merges, shapes in ((R.PLACE_MERGES, _geometry_shapes()), (RUN_MERGES, runs)):
        with _encoder(mode, merges) as enc:
            for name, (data, off), raw in shapes:
                _check(enc, mode, name, data, off, merges, raw)


@each_mode
def test_many_chunks_fuzz_pieces_and_16_bits(mode):
    data, off, merges = D.many_chunk_text()
    with _encoder(mode, merges) as enc:
        _check(enc, mode, "many chunks", data, off, merges, False)
        _check(enc, mode, "16-bit output", data, off, merges, False, dtype=np.uint16)
        enc.set_option("piece_bytes", 1800)                       # three pieces: the piece's base enters the instance
        _check(enc, mode, "three pieces", data, off, merges, False)
    f = R.fuzz_case(3, n_bytes=256 * 1024)
    with _encoder(mode, f.merges) as enc:
        _check(enc, mode, f.name, f.data.tobytes(), f.chunk_off, f.merges, boff=False)


@each_mode
def test_endmask_route(mode):
    dev = torch.device("cuda", 0)
    data, off = _text([n for n in _around(B - 40, B + 3) if n])
    tok, tok_off, byte_off = _reference(mode, data, off, R.PLACE_MERGES)
    d = DeviceCase(dev, data, off, np.arange(len(off)))
    with _encoder(mode, R.PLACE_MERGES) as enc:
        got, doc_tok = enc.encode_endmask(*d.ptrs(), doc_off=d.doc_off)
        assert np.array_equal(got, tok) and np.array_equal(doc_tok, tok_off)
        assert enc.n_passes == 1 and enc.resident_stats()["raw_tiles"] == 0
        got, _, boff = enc.encode_endmask(*d.ptrs(), byte_off=True)
        assert np.array_equal(got, tok) and np.array_equal(boff, byte_off)


@each_mode
def test_tokenizer_route_equals_the_host_loop(mode):
    pattern, _, merges = O.parse_model(read_golden("shakespeare_gpt4_lexical_512.model"))
    text = read_data("shakespeare.txt")[:40000]
    kw = dict(order=mode[0], dropout=mode[1], seed=SEED)
    t, docs = mbpe.Tokenizer(pattern), [text[:9000], b"", text[9000:]]
    t.set_merges(merges)
    assert np.array_equal(t.encode(text, device=0, resident=True, **kw), t.encode(text, **kw))
    got, want = t.encode_batch(docs, device=0, resident=True, **kw), [t.encode(d, **kw) for d in docs[:2]]
    assert all(np.array_equal(g, w) for g, w in zip(got, want)) and len(got) == 3    # (dropout: the third starts at 9,000)
    t.close()


def test_dedup_in_rank_order():
    mode, (data, off, merges) = ("rank", 0.0), D.many_chunk_text()
    tok, tok_off, _ = _reference(mode, data, off, merges)
    with _encoder(mode, merges, dedup=True) as enc:                # the stage runs over the unique chunks' text
        got, got_off = enc.encode(data, off, offsets=True)
        assert np.array_equal(got, tok) and np.array_equal(got_off, tok_off)
        dd, st = enc.dedup_stats(), enc.resident_stats()
        assert dd["n_unique"] < len(off) - 1 and enc.pass_tokens() == [dd["n_unique_bytes"]]
        assert st["raw_tiles"] == 0 and st["tokens_after_stage"] == dd["n_unique_tokens"] and enc.n_passes == 1


def test_option_on_off_on():
    mode, (data, off) = ("rank", 0.0), _text([7] * 150 + [3000] + [7] * 150)
    with mbpe.Encoder(R.PLACE_MERGES, rank_order=True) as enc:
        enc.set_option("resident", 1)
        _check(enc, mode, "on", data, off, R.PLACE_MERGES, True)
        enc.set_option("resident", 0)
        want = _reference(mode, data, off, R.PLACE_MERGES)
        got = enc.encode(data, off, offsets=True)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and enc.n_passes > 2
        with pytest.raises(mbpe.MbpeError):                       # (MBPE_ERR_STATE: the call did not run the stage)
            enc.resident_stats()
        enc.set_option("resident", 1)
        _check(enc, mode, "on again", data, off, R.PLACE_MERGES, True)
