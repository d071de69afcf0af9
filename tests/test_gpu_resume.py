"""Continuing a training from existing merges on the GPU: mbpe_train_begin_from / mbpe_train_from.

Expected values come from oracle.State: the prior merges are forced with merge(a, b, 256 + k), then top() / merge()
loop on.  The state tests look at what the begin leaves (slot stream in both layouts, pair table in both layouts);
the training tests hold a split or continued run to the uninterrupted oracle run.  Every training test asserts that
the oracle's counts stay >= 1: below that the reference merges zero-count pairs that only its history knows, which a
continuation cannot (mbpe.h)."""
import numpy as np
import pytest

import mbpe
import oracle as O
from conftest import read_data

pytestmark = pytest.mark.gpu

MODES = [("lexical", O.LEXICAL, 1), ("first", O.FIRST, 0)]      # name, oracle mode, conflict_resolution
LENGTHS = [0, 1, 2, 511, 512, 513, 1023, 1024, 1025, 2049, 4097]


def _rand16(n, seed):
    rng = np.random.RandomState(seed)
    return (rng.randint(0, 16, size=n) + 97).astype(np.uint8)


def _text(kind, n):
    """(bytes, chunk_off or None)"""
    if kind == "random16":
        return _rand16(n, 11 + n), None
    if kind == "run":
        return np.full(n, 97, dtype=np.uint8), None
    data = _rand16(n, 23 + n)
    if kind == "chunks1":
        return data, np.arange(n + 1, dtype=np.uint64)
    assert kind == "chunks1to7"
    # lengths 1..7 in a fixed irregular order; their sums pass 511 / 512 / 513 and 1023 / 1024 / 1025 in turn, and the
    # three offsets below put a chunk end exactly on slots 511 | 512 and 1023 | 1024 where the length allows
    rng = np.random.RandomState(5)
    cuts, at = {0, n}, 0
    while at < n:
        at += int(rng.randint(1, 8))
        if at < n:
            cuts.add(at)
    for c in (511, 512, 1023, 1024):
        if c < n:
            cuts.add(c)
    off = np.array(sorted(cuts), dtype=np.uint64)
    assert off[0] == 0 and off[-1] == n and (np.diff(off.astype(np.int64)) <= 7).all()
    return data, off


def _forced(data, off, omode, prior):
    st = O.State(data, off, mode=omode)
    for k, (a, b) in enumerate(prior):
        st.merge(int(a), int(b), 256 + k)
    return st


def _continue(st, k0, n_more):
    """top() / merge() from merge index k0 -> (merges, counts), stopping like the reference when no pair is left"""
    merges, counts = [], []
    for k in range(k0, k0 + n_more):
        top = st.top()
        if top is None:
            break
        a, b, c = top
        merges.append((a, b))
        counts.append(c)
        st.merge(a, b, 256 + k)
    return merges, counts


def _all_real_merges(data, off, omode):
    """every merge the oracle makes on this text while the chosen count is >= 1"""
    if len(data) < 2:
        return []
    m, c = O.train(data, 256 + len(data), off, mode=omode)
    n = 0
    while n < len(c) and c[n] >= 1:
        n += 1
    return [(int(a), int(b)) for a, b in m[:n]]


def _stream_of(st, chunked):
    tok, clen = st.stream()
    ends = np.zeros(len(tok), dtype=np.uint8)
    if chunked:
        last = np.cumsum(clen.astype(np.int64))[clen > 0] - 1
        ends[last] = 1
    return tok, ends


def _pairs_of(tok, ends):
    want = {}
    for i in range(len(tok) - 1):
        if not ends[i]:
            key = (int(tok[i]), int(tok[i + 1]))
            want[key] = want.get(key, 0) + 1
    return want


@pytest.mark.parametrize("kind", ["random16", "run", "chunks1to7", "chunks1"])
@pytest.mark.parametrize("mode", MODES, ids=[m[0] for m in MODES])
def test_state_after_begin(kind, mode):
    _, omode, cr = mode
    checked = 0
    with mbpe.Trainer(0) as tr:
        tr.set_option("conflict_resolution", cr)
        for n in LENGTHS:
            data, off = _text(kind, n)
            chunked = off is not None
            everything = _all_real_merges(data, off if n else None, omode)
            priors = {0: [], 1: everything[:1], 5: everything[:5], len(everything): everything}
            tr.load_corpus(data, off)
            for n_prior, prior in sorted(priors.items()):
                if n == 0:
                    want_tok, want_end = np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint8)
                else:
                    want_tok, want_end = _stream_of(_forced(data, off, omode, prior), chunked)
                want_pairs = _pairs_of(want_tok, want_end)
                for dense in (1, 0):
                    for barrier in ((0, 1) if chunked else (0,)):
                        tr.set_option("dense_table", dense)
                        tr.set_option("chunk_barrier", barrier)
                        tr.train_begin(256 + len(prior) + 4, prior_merges=np.array(prior, dtype=np.uint32).reshape(-1, 2))
                        tag = (kind, n, n_prior, "dense" if dense else "hashed", "barrier" if barrier else "endbit")
                        tok, end = tr.stream()
                        assert tok.tolist() == want_tok.tolist(), tag
                        assert end.tolist() == want_end.tolist(), tag
                        assert tr.pairs_dict() == want_pairs, tag
                        st = tr.stats()
                        assert st["n_live"] == len(want_tok) and st["n_pairs"] == len(want_pairs), (tag, st)
                        assert st["n_merges"] == len(prior), (tag, st)
                        checked += 1
    assert checked >= len(LENGTHS) * 3 * 2


# ---- split training equals whole training ---------------------------------------------------------------------

SPLITS = [0, 1, 37, 143, 255]


def _corpus(name):
    if name == "taylor_basic":
        return np.frombuffer(read_data("taylorswift.txt"), dtype=np.uint8), None
    if name == "taylor_gpt4":
        data = read_data("taylorswift.txt")
        return np.frombuffer(data, dtype=np.uint8), mbpe.presplit(O.PATTERNS["gpt4"], data)
    assert name == "splitmix64k"
    return O.splitmix64_bytes(42, 1 << 16), None


_whole = {}


def _oracle_whole(name, omode):
    """the uninterrupted oracle run to vocab 512, once per corpus and mode"""
    if (name, omode) not in _whole:
        data, off = _corpus(name)
        m, c = O.train(data, 512, off, mode=omode)
        assert len(m) == 256 and int(c.min()) >= 1, (name, omode, len(m), int(c.min()))
        _whole[(name, omode)] = (data, off, m, c)
    return _whole[(name, omode)]


def _assert_continued(got_m, got_c, want_m, want_c, split, tag):
    assert got_m.tolist() == want_m.tolist(), tag
    assert got_c[:split].tolist() == [-1] * split, tag
    assert got_c[split:].tolist() == want_c[split:].tolist(), tag


@pytest.mark.parametrize("name", ["taylor_basic", "taylor_gpt4", "splitmix64k"])
@pytest.mark.parametrize("mode", MODES, ids=[m[0] for m in MODES])
def test_split_equals_whole(name, mode):
    _, omode, cr = mode
    data, off, want_m, want_c = _oracle_whole(name, omode)
    print(name, mode[0], "lowest oracle count", int(want_c.min()))
    with mbpe.Trainer(0) as tr:
        whole_m, whole_c, _ = tr.train(data, 512, off, conflict_resolution=cr)
        assert whole_m.tolist() == want_m.tolist() and whole_c.tolist() == want_c.tolist()
        for split in SPLITS:
            got_m, got_c, st = tr.train(data, 512, off, conflict_resolution=cr, prior_merges=want_m[:split])
            _assert_continued(got_m, got_c, want_m, want_c, split, (name, mode[0], split))
            assert st["n_merges"] == 256
        # the same split through the step-level calls: new merges are counted, prior ones are not
        tr.set_option("conflict_resolution", cr)
        tr.load_corpus(data, off)
        tr.train_begin(512, prior_merges=want_m[:143])
        assert tr.train_steps(10) == 10
        assert tr.train_steps(1000) == 256 - 143 - 10
        got_m, got_c = tr.train_result()
        _assert_continued(got_m, got_c, want_m, want_c, 143, (name, mode[0], "steps"))


@pytest.mark.parametrize("mode", MODES, ids=[m[0] for m in MODES])
def test_split_twice_and_loop_options(mode):
    _, omode, cr = mode
    data, off, want_m, want_c = _oracle_whole("taylor_gpt4", omode)
    with mbpe.Trainer(0) as tr:
        a_m, a_c, _ = tr.train(data, 256 + 37, off, conflict_resolution=cr)                       # A
        assert a_m.tolist() == want_m[:37].tolist()
        b_m, b_c, _ = tr.train(data, 256 + 143, off, conflict_resolution=cr, prior_merges=a_m)      # A -> B
        _assert_continued(b_m, b_c, want_m[:143], want_c[:143], 37, "A->B")
        c_m, c_c, _ = tr.train(data, 512, off, conflict_resolution=cr, prior_merges=b_m)            # B -> C
        _assert_continued(c_m, c_c, want_m, want_c, 143, "B->C")
    for opt, val in (("multi_merge", 0), ("fused_min", 2)):
        for layout in (("dense_table", 0), ("chunk_barrier", 1)):
            with mbpe.Trainer(0) as tr:
                tr.set_option(opt, val)
                tr.set_option(*layout)
                got_m, got_c, st = tr.train(data, 512, off, conflict_resolution=cr, prior_merges=want_m[:37])
                _assert_continued(got_m, got_c, want_m, want_c, 37, (opt, layout))
                if opt == "fused_min" and cr == 1:
                    assert st["n_fused"] >= 1, st          # fused passes did run on the resumed stream


# ---- another corpus -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(144, 156, 1 << 16), (50, 40, 1 << 12)], ids=["144+156 on 64KiB", "50+40 on 4KiB"])
@pytest.mark.parametrize("mode", MODES, ids=[m[0] for m in MODES])
def test_another_corpus(shape, mode):
    n_prior, n_more, n_bytes = shape
    _, omode, cr = mode
    taylor = np.frombuffer(read_data("taylorswift.txt"), dtype=np.uint8)
    prior, _ = O.train(taylor, 256 + n_prior, None, mode=omode)
    assert len(prior) == n_prior
    text = np.frombuffer(read_data("shakespeare.txt")[:n_bytes], dtype=np.uint8)
    st = _forced(text, None, omode, prior)
    begin_tok, _ = st.stream()
    absent = set(range(256, 256 + n_prior)) - set(begin_tok.tolist())
    assert absent, "every prior merge occurs in the new text: the case tests nothing"
    want_m, want_c = _continue(st, n_prior, n_more)
    assert len(want_m) == n_more and min(want_c) >= 1, (len(want_m), min(want_c))
    print(shape, mode[0], "lowest oracle count", min(want_c), "prior ids absent from the new text", len(absent))
    for dense in (1, 0):
        with mbpe.Trainer(0) as tr:
            tr.set_option("conflict_resolution", cr)
            tr.set_option("dense_table", dense)
            tr.load_corpus(text)
            tr.train_begin(256 + n_prior + n_more, prior_merges=prior)
            tok, _ = tr.stream()
            assert tok.tolist() == begin_tok.tolist()
            assert not (absent & set(tok.tolist()))
            assert tr.train_steps(n_more) == n_more
            got_m, got_c = tr.train_result()
            assert got_m[:n_prior].tolist() == prior.tolist()
            assert [tuple(p) for p in got_m[n_prior:].tolist()] == want_m
            assert got_c.tolist() == [-1] * n_prior + want_c
            want_tok, _ = st.stream()
            assert tr.stream()[0].tolist() == want_tok.tolist()
            assert tr.decode_stream() == text.tobytes()


# ---- ends -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES, ids=[m[0] for m in MODES])
def test_ends(mode):
    _, omode, cr = mode
    data, off = _text("chunks1to7", 1025)
    everything = np.array(_all_real_merges(data, off, omode), dtype=np.uint32).reshape(-1, 2)
    assert len(everything) > 5
    with mbpe.Trainer(0) as tr:
        tr.set_option("conflict_resolution", cr)
        # a prior table that leaves nothing to merge: the begin is fine, no merge follows, the result is the table
        left = _forced(data, off, omode, everything)
        assert not _pairs_of(*_stream_of(left, True))
        tr.load_corpus(data, off)
        tr.train_begin(256 + len(everything) + 10, prior_merges=everything)
        assert tr.train_steps(10) == 0
        m, c = tr.train_result()
        assert m.tolist() == everything.tolist() and c.tolist() == [-1] * len(everything)
        assert tr.stats()["n_merges"] == len(everything)
        assert tr.decode_stream() == data.tobytes()
        # n_prior == vocab_size - 256: complete at once
        tr.train_begin(256 + 5, prior_merges=everything[:5])
        assert tr.train_steps(10) == 0 and tr.train_sequences(10) == 0
        m, c = tr.train_result()
        assert m.tolist() == everything[:5].tolist() and c.tolist() == [-1] * 5
        # a resumed training that runs: the stream decodes to the corpus
        tr.train_begin(256 + 12, prior_merges=everything[:5])
        assert tr.train_steps(100) == 7
        m, c = tr.train_result()
        assert m.tolist() == everything[:12].tolist() and c[:5].tolist() == [-1] * 5 and (c[5:] >= 1).all()
        tr.compact()
        assert tr.decode_stream() == data.tobytes()
        # the one-call form hands the same back
        m2, c2, _ = tr.train(data, 256 + 12, off, conflict_resolution=cr, prior_merges=everything[:5])
        assert m2.tolist() == m.tolist() and c2.tolist() == c.tolist()


# ---- errors ---------------------------------------------------------------------------------------------------

def _code(fn, *a, **kw):
    with pytest.raises(mbpe.MbpeError) as e:
        fn(*a, **kw)
    return e.value.code


def test_errors():
    data, off = _text("chunks1to7", 513)
    good = np.array(_all_real_merges(data, off, O.LEXICAL)[:5], dtype=np.uint32)
    # 65,536 distinct byte pairs: a valid table of any length up to that
    long_table = np.array([[k >> 8, k & 255] for k in range(40000)], dtype=np.uint32)
    with mbpe.Trainer(0) as tr:
        tr.load_corpus(data, off)
        assert _code(tr.train_begin, 300, prior_merges=[[97, 98], [97, 98]]) == mbpe.ERR_ARG          # repeated pair
        assert _code(tr.train_begin, 300, prior_merges=[[97, 98], [258, 98]]) == mbpe.ERR_ARG         # forward reference
        assert _code(tr.train_begin, 256 + 4, prior_merges=good) == mbpe.ERR_ARG                      # n_prior too large
        tr.set_option("chunk_barrier", 0)                                                              # end-bit slots: 32,766 ids
        assert _code(tr.train_begin, 32767, prior_merges=good) == mbpe.ERR_VOCAB
        assert _code(tr.train_begin, 32767, prior_merges=long_table[:32767 - 256]) == mbpe.ERR_VOCAB
        tr.set_option("chunk_barrier", -1)
        assert _code(tr.train_begin, 65519, prior_merges=good) == mbpe.ERR_VOCAB                       # beyond the barrier layout
        tr.set_option("wide_from", 3)
        assert _code(tr.train_begin, 300, prior_merges=good) == mbpe.ERR_VOCAB
        tr.set_option("wide_from", -1)
        tr.comm_init_external(0, 2)
        assert _code(tr.train_begin, 300, prior_merges=good) == mbpe.ERR_STATE
        tr.comm_init_external(0, 1)
        # none of it left a trace: the context trains normally, from bytes and from the table
        want_m, want_c = O.train(data, 300, off)
        tr.train_begin(300)
        assert tr.train_steps(44) == 44
        m, c = tr.train_result()
        assert m.tolist() == want_m.tolist() and c.tolist() == want_c.tolist()
        tr.train_begin(300, prior_merges=good)
        tr.train_steps(44)
        m, c = tr.train_result()
        assert m.tolist() == want_m.tolist() and c[5:].tolist() == want_c[5:].tolist()
    with mbpe.Trainer(0) as tr:                                  # one chunk: 65,534 ids
        tr.load_corpus(data)
        assert _code(tr.train_begin, 65535, prior_merges=good) == mbpe.ERR_VOCAB
    with mbpe.Trainer(0) as tr:                                  # call order: no corpus
        assert _code(tr.train_begin, 300, prior_merges=good) == mbpe.ERR_STATE
