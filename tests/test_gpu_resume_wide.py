"""Continuing a training from existing merges beyond the 16-bit slot format: option "resume_wide" of
mbpe_train_begin_from.  With h the merge at which the slot stream hands over (the format's limit, or "wide_from") and
T = vocab_size - 256: T <= h is the slot case of test_gpu_resume.py, n_prior < h < T the mixed case (the begin on the
slot stream, the handover of test_gpu_wide.py at merge h), n_prior >= h the direct case -- the replay's tokens are the
32-bit stream and k_wide_pair_count_tokens counts the 64-bit-key table from them.

Expected values as in test_gpu_resume.py: oracle.State with the prior merges forced, or the uninterrupted oracle run;
every training test asserts that the counts it compares stay >= 1 (the zero-count divergence of DESIGN.md 4h).  Only
the last test's reference is the uninterrupted DEVICE training, which test_gpu_wide.py pins to the oracle on the very
same corpus."""
import numpy as np
import pytest

import mbpe
import oracle as O
from conftest import read_data
from test_gpu_resume import (MODES, _all_real_merges, _assert_continued, _code, _continue, _forced, _pairs_of, _stream_of,
                             _text)
from test_gpu_wide import _word_corpus

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 2, 1023, 1024, 1025, 2049, 4097]      # the 1,024-token span edges of the 32-bit loop
KINDS = ["random16", "run", "chunks1to7", "chunks1"]
NEVER = [(1, 2), (256, 3)]                              # valid merges of bytes that no text here holds


def _trainer(cr):
    tr = mbpe.Trainer(0)
    tr.set_option("conflict_resolution", cr)
    tr.set_option("first_wide", 1)
    tr.set_option("resume_wide", 1)
    return tr


def _arr(prior):
    return np.array(prior, dtype=np.uint32).reshape(-1, 2)


def _recount(tr):
    """the pairs of the live stream, counted with numpy -> {(a, b): count}"""
    tok, end = tr.stream()
    if len(tok) < 2:
        return {}
    keep = end[:-1] == 0
    keys = (tok[:-1].astype(np.uint64) << np.uint64(32)) | tok[1:].astype(np.uint64)
    u, n = np.unique(keys[keep], return_counts=True)
    return {(int(k >> np.uint64(32)), int(k & np.uint64(0xFFFFFFFF))): int(c) for k, c in zip(u, n)}


# ---- state after a direct begin -------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", MODES, ids=[m[0] for m in MODES])
def test_state_after_direct_begin(kind, mode):
    _, omode, cr = mode
    checked = 0
    with _trainer(cr) as tr:
        for n in LENGTHS:
            data, off = _text(kind, n)
            chunked = off is not None
            # (a text without a pair -- one token per chunk, or shorter than two bytes -- takes a table that never applies)
            everything = _all_real_merges(data, off if n else None, omode) or NEVER
            priors = {1: everything[:1], 5: everything[:5], len(everything): everything}
            tr.load_corpus(data, off)
            for n_prior, prior in sorted(priors.items()):
                if n == 0:
                    want_tok, want_end = np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint8)
                else:
                    want_tok, want_end = _stream_of(_forced(data, off, omode, prior), chunked)
                want_pairs = _pairs_of(want_tok, want_end)
                for wide_from in sorted({0, len(prior) - 1, len(prior)}):      # len(prior): the last direct one
                    tr.set_option("wide_from", wide_from)
                    tr.train_begin(256 + len(prior) + 4, prior_merges=_arr(prior))
                    tag = (kind, n, n_prior, wide_from)
                    tok, end = tr.stream()
                    assert tok.tolist() == want_tok.tolist(), tag
                    assert end.tolist() == want_end.tolist(), tag
                    assert tr.pairs_dict() == want_pairs, tag
                    st = tr.stats()
                    assert st["n_live"] == len(want_tok) and st["n_pairs"] == len(want_pairs), (tag, st)
                    assert st["n_merges"] == len(prior), (tag, st)
                    m, c = tr.train_result()
                    assert m.tolist() == _arr(prior).tolist() and c.tolist() == [-1] * len(prior), tag
                    checked += 1
    assert checked >= len(LENGTHS) * 2


@pytest.mark.parametrize("name", ["splitmix64k", "run"])
def test_direct_begin_cache_paths(name):
    """64 KiB of SplitMix64 bytes: far more distinct pairs than LDS entries, most positions miss the cache and go to
    the table directly.  A run: one key takes every count of every workgroup's cache."""
    if name == "splitmix64k":
        data = O.splitmix64_bytes(42, 1 << 16)
        prior = [(int(a), int(b)) for a, b in O.train(data, 256 + 5)[0]]
    else:
        data = np.full(70000, 97, dtype=np.uint8)
        prior = [(97, 97)]
    with _trainer(1) as tr:
        tr.set_option("wide_from", 0)
        tr.load_corpus(data)
        tr.train_begin(256 + len(prior) + 4, prior_merges=_arr(prior))
        want = _recount(tr)
        assert tr.pairs_dict() == want
        want_tok, _ = _forced(data, None, O.LEXICAL, prior).stream()
        assert tr.stream()[0].tolist() == want_tok.tolist()
        if name == "run":
            assert want == {(256, 256): 35000 - 1}
        else:
            assert len(want) > 8 * 1024


# ---- mixed begin ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", MODES, ids=[m[0] for m in MODES])
def test_mixed_begin_steps_across_the_handover(kind, mode):
    _, omode, cr = mode
    checked = 0
    with _trainer(cr) as tr:
        for n in (1025, 4097):
            data, off = _text(kind, n)
            chunked = off is not None
            everything = _all_real_merges(data, off, omode)
            tr.load_corpus(data, off)
            if not everything:
                # one token per chunk: no pair, before or after any merge -- the begin succeeds and nothing follows
                assert kind == "chunks1"
                for barrier in (0, 1):
                    tr.set_option("wide_from", 4)
                    tr.set_option("chunk_barrier", barrier)
                    tr.train_begin(256 + 8, prior_merges=_arr(NEVER))
                    assert tr.train_steps(3) == 0
                    m, c = tr.train_result()
                    assert m.tolist() == _arr(NEVER).tolist() and c.tolist() == [-1, -1]
                    assert tr.stream()[0].tolist() == data.tolist() and tr.pairs_dict() == {}
                    checked += 1
                continue
            assert len(everything) >= 11, (kind, n, len(everything))
            for n_prior in (1, 5):
                prior = everything[:n_prior]
                for wide_from in (n_prior + 1, n_prior + 3):
                    for barrier in ((0, 1) if chunked else (0,)):
                        tr.set_option("wide_from", wide_from)
                        tr.set_option("chunk_barrier", barrier)
                        n_more = 6
                        tr.train_begin(256 + n_prior + n_more, prior_merges=_arr(prior))
                        st = _forced(data, off, omode, prior)
                        for k in range(n_prior, n_prior + n_more):
                            tag = (kind, n, n_prior, wide_from, barrier, k)
                            a, b, cnt = st.top()
                            st.merge(a, b, 256 + k)
                            assert cnt >= 1, tag
                            assert tr.train_steps(1) == 1, tag
                            m, c = tr.train_result()
                            assert m[-1].tolist() == [a, b] and int(c[-1]) == cnt and len(m) == k + 1, tag
                            want_tok, want_end = _stream_of(st, chunked)
                            tok, end = tr.stream()
                            assert tok.tolist() == want_tok.tolist() and end.tolist() == want_end.tolist(), tag
                            got = {p: v for p, v in tr.pairs_dict().items() if v}
                            assert got == _pairs_of(want_tok, want_end), tag
                            checked += 1
                        assert tr.stream_device()[2] == 32      # (the handover took place)
    assert checked


# ---- split training equals whole training ---------------------------------------------------------------------

VOCAB = 256 + 120
_whole = {}


def _corpus(name):
    if name in ("taylor_gpt2", "taylor_gpt4"):
        data = read_data("taylorswift.txt")[20000:50000]
        return np.frombuffer(data, dtype=np.uint8), mbpe.presplit(O.PATTERNS[name[-4:]], data)
    assert name == "random4"
    return (np.random.RandomState(9).randint(0, 4, size=8192) + 97).astype(np.uint8), None


def _oracle_whole(name, omode):
    if (name, omode) not in _whole:
        data, off = _corpus(name)
        m, c = O.train(data, VOCAB, off, mode=omode)
        assert len(m) == VOCAB - 256 and int(c.min()) >= 1, (name, omode, len(m), int(c.min()))
        _whole[(name, omode)] = (data, off, m, c)
    return _whole[(name, omode)]


@pytest.mark.parametrize("name", ["taylor_gpt2", "taylor_gpt4", "random4"])
@pytest.mark.parametrize("mode", MODES, ids=[m[0] for m in MODES])
def test_split_equals_whole(name, mode):
    _, omode, cr = mode
    data, off, want_m, want_c = _oracle_whole(name, omode)
    with _trainer(cr) as tr:
        for split in (1, 37, 119):
            for wide_from in (0, 20, split, split + 5, 200):      # direct, direct or mixed, direct, mixed, slot case
                tr.set_option("wide_from", wide_from)
                got_m, got_c, st = tr.train(data, VOCAB, off, conflict_resolution=cr, prior_merges=want_m[:split])
                tag = (name, mode[0], split, wide_from)
                _assert_continued(got_m, got_c, want_m, want_c, split, tag)
                assert st["n_merges"] == VOCAB - 256, tag
                assert tr.decode_stream() == data.tobytes(), tag
        # the step-level calls: new merges are counted, prior ones are not
        for wide_from in (0, 42):                                  # direct; mixed with the handover inside the first call
            tr.set_option("wide_from", wide_from)
            tr.load_corpus(data, off)
            tr.train_begin(VOCAB, prior_merges=want_m[:37])
            assert tr.train_steps(10) == 10
            assert tr.train_steps(1000) == 120 - 37 - 10
            got_m, got_c = tr.train_result()
            _assert_continued(got_m, got_c, want_m, want_c, 37, (name, mode[0], "steps", wide_from))
        # A -> B -> C, the direct case in both continuations
        tr.set_option("wide_from", 0)
        a_m = want_m[:37]
        b_m, b_c, _ = tr.train(data, 256 + 80, off, conflict_resolution=cr, prior_merges=a_m)
        _assert_continued(b_m, b_c, want_m[:80], want_c[:80], 37, "A->B")
        c_m, c_c, _ = tr.train(data, VOCAB, off, conflict_resolution=cr, prior_merges=b_m)
        _assert_continued(c_m, c_c, want_m, want_c, 80, "B->C")


# ---- ends -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES, ids=[m[0] for m in MODES])
def test_ends(mode):
    _, omode, cr = mode
    data, off = _text("chunks1to7", 1025)
    everything = _arr(_all_real_merges(data, off, omode))
    assert len(everything) > 5
    with _trainer(cr) as tr:
        tr.set_option("wide_from", 0)
        # a prior table that leaves no pair at all: the begin is fine, the loop ends at once, the result is the table
        assert not _pairs_of(*_stream_of(_forced(data, off, omode, everything), True))
        tr.load_corpus(data, off)
        tr.train_begin(256 + len(everything) + 10, prior_merges=everything)
        assert tr.train_steps(10) == 0
        m, c = tr.train_result()
        assert m.tolist() == everything.tolist() and c.tolist() == [-1] * len(everything)
        assert tr.stats()["n_merges"] == len(everything)
        assert tr.decode_stream() == data.tobytes()
        # n_prior == vocab_size - 256 is the slot case (T <= h needs h >= 5) ...
        tr.set_option("wide_from", 5)
        tr.train_begin(256 + 5, prior_merges=everything[:5])
        assert tr.train_steps(10) == 0 and tr.train_sequences(10) == 0
        m, c = tr.train_result()
        assert m.tolist() == everything[:5].tolist() and c.tolist() == [-1] * 5
        # ... and the direct case below it
        tr.set_option("wide_from", 2)
        tr.train_begin(256 + 5, prior_merges=everything[:5])
        assert tr.train_steps(10) == 0 and tr.train_sequences(10) == 0
        m, c = tr.train_result()
        assert m.tolist() == everything[:5].tolist() and c.tolist() == [-1] * 5
        assert tr.decode_stream() == data.tobytes()
        # empty text
        tr.load_corpus(np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64))
        tr.train_begin(256 + 9, prior_merges=everything[:5])
        assert tr.train_steps(10) == 0
        m, c = tr.train_result()
        assert m.tolist() == everything[:5].tolist() and c.tolist() == [-1] * 5
        assert len(tr.stream()[0]) == 0 and tr.pairs_dict() == {} and tr.decode_stream() == b""


# ---- another corpus -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES, ids=[m[0] for m in MODES])
def test_another_corpus(mode):
    n_prior, n_more, n_bytes = 50, 40, 1 << 12
    _, omode, cr = mode
    taylor = np.frombuffer(read_data("taylorswift.txt"), dtype=np.uint8)
    prior, _ = O.train(taylor, 256 + n_prior, None, mode=omode)
    assert len(prior) == n_prior
    text = np.frombuffer(read_data("shakespeare.txt")[:n_bytes], dtype=np.uint8)
    st = _forced(text, None, omode, prior)
    begin_tok, _ = st.stream()
    absent = set(range(256, 256 + n_prior)) - set(begin_tok.tolist())
    assert absent, "every prior merge occurs in the new text: the case tests nothing"
    begin_pairs = _pairs_of(begin_tok, np.zeros(len(begin_tok), dtype=np.uint8))
    want_m, want_c = _continue(st, n_prior, n_more)
    assert len(want_m) == n_more and min(want_c) >= 1, (len(want_m), min(want_c))
    with _trainer(cr) as tr:
        tr.set_option("wide_from", 0)
        tr.load_corpus(text)
        tr.train_begin(256 + n_prior + n_more, prior_merges=prior)
        tok, _ = tr.stream()
        assert tok.tolist() == begin_tok.tolist()
        assert not (absent & set(tok.tolist()))
        assert tr.pairs_dict() == begin_pairs
        assert tr.train_steps(n_more) == n_more
        got_m, got_c = tr.train_result()
        assert got_m[:n_prior].tolist() == prior.tolist()
        assert [tuple(p) for p in got_m[n_prior:].tolist()] == want_m
        assert got_c.tolist() == [-1] * n_prior + want_c
        want_tok, _ = st.stream()
        assert tr.stream()[0].tolist() == want_tok.tolist()
        assert {p: v for p, v in tr.pairs_dict().items() if v} == _pairs_of(want_tok, np.zeros(len(want_tok), dtype=np.uint8))
        assert tr.decode_stream() == text.tobytes()


# ---- ids really beyond 16 bits --------------------------------------------------------------------------------

def test_ids_beyond_16_bits():
    """Reference: the uninterrupted device training to 68,000 (tests/test_gpu_wide.py holds exactly this run to the
    oracle).  Continued from its first 66,000 - 256 merges (direct: 17-bit ids among the prior merges and in the
    replay) and from its first 60,000 - 256 (mixed: handover at id 65,518)."""
    data, off = _word_corpus(78, 4200, 24, (6, 14))
    vocab = 68000
    with mbpe.Trainer(0) as tr:
        want_m, want_c, _ = tr.train_lexical(data, vocab, off)
        want_tok, want_end = tr.stream()
    assert len(want_m) == vocab - 256 and int(want_c.min()) >= 2 and int(want_m.max()) > 65535
    with _trainer(1) as tr:
        for first_n in (66000 - 256, 60000 - 256):
            prior = want_m[:first_n]
            if first_n == 66000 - 256:
                assert int(prior.max()) > 65535
            got_m, got_c, st = tr.train(data, vocab, off, conflict_resolution=1, prior_merges=prior)
            _assert_continued(got_m, got_c, want_m, want_c, first_n, first_n)
            tok, end = tr.stream()
            assert np.array_equal(tok, want_tok) and np.array_equal(end, want_end), first_n
            assert {p: v for p, v in tr.pairs_dict().items() if v} == _recount(tr), first_n
            assert tr.decode_stream() == data.tobytes(), first_n


# ---- errors ---------------------------------------------------------------------------------------------------

def test_errors():
    data, off = _text("chunks1to7", 513)
    good = _arr(_all_real_merges(data, off, O.LEXICAL)[:5])
    long_table = np.array([[k >> 8, k & 255] for k in range(40000)], dtype=np.uint32)
    want_m, want_c = O.train(data, 300, off)

    def trains_normally(tr):
        tr.train_begin(300)
        assert tr.train_steps(44) == 44
        m, c = tr.train_result()
        assert m.tolist() == want_m.tolist() and c.tolist() == want_c.tolist()
        tr.train_begin(300, prior_merges=good)
        tr.train_steps(44)
        m, c = tr.train_result()
        assert m.tolist() == want_m.tolist() and c[5:].tolist() == want_c[5:].tolist()

    with mbpe.Trainer(0) as tr:
        tr.load_corpus(data, off)
        # two ranks, option on (the transport can only change before the context's first begin)
        tr.set_option("resume_wide", 1)
        tr.comm_init_external(0, 2)
        assert _code(tr.train_begin, 65519, prior_merges=good) == mbpe.ERR_STATE
        tr.set_option("wide_from", 0)
        assert _code(tr.train_begin, 300, prior_merges=good) == mbpe.ERR_STATE
        tr.set_option("wide_from", -1)
        tr.comm_init_external(0, 1)
        tr.set_option("resume_wide", 0)
        # the default: "resume_wide" 0, every refusal of a begin beyond the slot format as it was
        tr.set_option("chunk_barrier", 0)
        assert _code(tr.train_begin, 32767, prior_merges=good) == mbpe.ERR_VOCAB
        assert _code(tr.train_begin, 32767, prior_merges=long_table[:32767 - 256]) == mbpe.ERR_VOCAB
        tr.set_option("chunk_barrier", -1)
        assert _code(tr.train_begin, 65519, prior_merges=good) == mbpe.ERR_VOCAB
        tr.set_option("wide_from", 3)
        assert _code(tr.train_begin, 300, prior_merges=good) == mbpe.ERR_VOCAB
        tr.set_option("wide_from", -1)
        trains_normally(tr)
        assert _code(tr.set_option, "resume_wide", 2) == mbpe.ERR_ARG
        assert _code(tr.set_option, "resume_wide", -1) == mbpe.ERR_ARG
        tr.set_option("resume_wide", 1)
        tr.set_option("conflict_resolution", 0)                    # `first` without "first_wide"
        assert _code(tr.train_begin, 65519, prior_merges=good) == mbpe.ERR_VOCAB
        tr.set_option("wide_from", 3)
        assert _code(tr.train_begin, 300, prior_merges=good) == mbpe.ERR_VOCAB
        tr.set_option("wide_from", -1)
        tr.set_option("conflict_resolution", 1)
        trains_normally(tr)
        assert _code(tr.train_begin, (1 << 24) + 1, prior_merges=good) == mbpe.ERR_VOCAB
        trains_normally(tr)
        # and with the option on, the vocabulary that was refused begins
        tr.train_begin(65519, prior_merges=good)
        assert tr.stats()["n_merges"] == 5
