"""The `first` tie-break (the reference CLI's default: PairCountInsertOrder, PairCount.h:55-181; table rebuilt before
every merge, Tokenizer.h:557-589) beyond the 16-bit slot format: with the option "first_wide" the training continues
on 32-bit tokens (csrc/wide.h) and settles ties there by the earliest first occurrence in the stream, ending when no
pair is left.  Step parity against the oracle across the hand-over, whole trainings, the end of the loop, ids past
65,535 checked by exact recount, a tie beyond token 2^32, and the CLI's default command line."""
import os
import subprocess

import numpy as np
import pytest

import mbpe
import oracle as O
from conftest import DATA, ROOT, read_data
from test_gpu_parity import _defaults, _random_chunks
from test_gpu_wide import _word_corpus

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "minbpe-cc_amd", "minbpe-cc")


@pytest.fixture(scope="module")
def tr():
    t = mbpe.Trainer(0)
    yield t
    t.close()


def _reset(tr):
    _defaults(tr)
    tr.set_option("conflict_resolution", 1)
    tr.set_option("first_wide", 0)


def _first_step_parity(tr, data, off, vocab, wide_from, **opts):
    """One merge per call, `first` mode, hand-over after `wide_from` merges: after every step the chosen pair and its
    count, the live stream, the chunk ends and the nonzero pair table against O.State(mode=O.FIRST)."""
    for k, v in opts.items():
        tr.set_option(k, v)
    tr.set_option("conflict_resolution", 0)
    tr.set_option("first_wide", 1)
    tr.set_option("wide_from", wide_from)
    st = O.State(data, off, mode=O.FIRST)
    try:
        tr.load_corpus(data, off)
        tr.train_begin(vocab)
        for i in range(vocab - 256):
            top = st.top()
            done = tr.train_steps(1)
            if top is None:                     # no pair left: the reference's loop breaks (Tokenizer.h:586-588)
                assert done == 0, "step %d" % i
                assert len(tr.train_result()[0]) == i
                assert tr.stats()["n_merges"] == i
                break
            assert done == 1, "step %d" % i
            m, c = tr.train_result()
            assert len(m) == i + 1
            assert (int(m[i][0]), int(m[i][1]), int(c[i])) == top, "step %d" % i
            st.merge(top[0], top[1], 256 + i)
            want_toks, want_clen = st.stream()
            toks, ends = tr.stream()
            assert np.array_equal(toks, want_toks), "stream differs at step %d" % i
            if off is not None:
                pos = np.cumsum(want_clen[want_clen > 0]).astype(np.int64) - 1
                want_ends = np.zeros(len(want_toks), dtype=np.uint8)
                want_ends[pos] = 1
                assert np.array_equal(ends, want_ends), "chunk ends differ at step %d" % i
            want_tab = {k_: v_ for k_, v_ in st.table_dict().items() if v_}
            got_tab = {k_: v_ for k_, v_ in tr.pairs_dict().items() if v_}
            assert got_tab == want_tab, "pair table differs at step %d" % i
    finally:
        st.close()
        _reset(tr)


# ---- 1. step parity across the hand-over ------------------------------------------------------------------------

@pytest.mark.parametrize("seed", range(8))
def test_first_step_parity_small_alphabet_wide(tr, seed):
    # 1-4 symbols: ties on nearly every merge, runs (a == b), touching matches, candidates across 1,024-token spans
    rng = np.random.default_rng(500 + seed)
    n = int(rng.integers(1, 9000))
    data = rng.integers(97, 97 + int(rng.integers(1, 5)), size=n, dtype=np.uint8)
    _first_step_parity(tr, data, None, 256 + 40, int(rng.integers(0, 13)), batch=1)


@pytest.mark.parametrize("seed", range(8))
def test_first_step_parity_chunked_wide(tr, seed):
    # chunk ends as flag bits and as barrier slots before the conversion; no pair crosses a chunk end
    rng = np.random.default_rng(600 + seed)
    n = int(rng.integers(2, 9000))
    data = rng.integers(97, 97 + int(rng.integers(1, 6)), size=n, dtype=np.uint8)
    off = _random_chunks(rng, n, int(rng.integers(2, 12)))
    _first_step_parity(tr, data, off, 256 + 40, int(rng.integers(0, 13)), batch=1, chunk_barrier=seed % 2)


def test_first_step_parity_runs_across_spans_wide(tr):
    # long runs over several spans, chunk ends at span edges: first occurrences sit right at span boundaries
    data = np.frombuffer(b"a" * 5000 + b"ab" * 3000 + b"aab" * 1000, dtype=np.uint8)
    cuts = sorted(set([1023, 1024, 1025, 2047, 2048, 2049, 4096, 5000, 5001, 7000, 9000, 11001]))
    off = np.array([0] + cuts + [len(data)], dtype=np.uint64)
    _first_step_parity(tr, data, None, 256 + 30, 0, batch=1)
    _first_step_parity(tr, data, off, 256 + 30, 0, batch=1)
    _first_step_parity(tr, data, off, 256 + 30, 3, batch=1, chunk_barrier=1)


# ---- 2. whole trainings ------------------------------------------------------------------------------------------

def _tie_broken_by_position(data, off, merges, start):
    """Is there a merge at index >= start where several pairs share the maximal count and the one taken is not the
    lexical winner among them?  (Replays `merges` on an oracle state.)"""
    st = O.State(data, off, mode=O.FIRST)
    try:
        for i, (a, b) in enumerate(merges):
            if i >= start:
                tab = st.table_dict()
                top = max(tab.values())
                tied = sorted(k for k, v in tab.items() if v == top)
                if len(tied) > 1 and tied[0] != (int(a), int(b)):
                    return True
            st.merge(int(a), int(b), 256 + i)
    finally:
        st.close()
    return False


@pytest.mark.parametrize("seed", range(4))
def test_first_whole_training_text_wide(tr, seed):
    data = read_data("taylorswift.txt")[seed * 20000:seed * 20000 + 30000]
    off = mbpe.presplit(O.GPT4_SPLIT_PATTERN if seed % 2 else O.GPT2_SPLIT_PATTERN, data)
    vocab, wf = 256 + 150, 40 + 10 * seed
    want_m, want_c = O.train(data, vocab, off, mode=O.FIRST)
    tr.set_option("first_wide", 1)
    tr.set_option("wide_from", wf)
    try:
        m, c, st = tr.train(data, vocab, off, conflict_resolution=0)     # (mbpe_train takes the context's first_wide)
    finally:
        _reset(tr)
    assert m.tolist() == want_m.tolist() and c.tolist() == want_c.tolist()
    assert st["n_merges"] == len(want_m)
    lex_m, _ = O.train(data, vocab, off)
    assert lex_m.tolist() != want_m.tolist()
    assert _tie_broken_by_position(data, off, want_m, wf)      # the 32-bit loop itself took a non-lexical tie


# ---- 3. the loop ends like the reference's -----------------------------------------------------------------------

@pytest.mark.parametrize("chunked", [False, True])
def test_first_wide_loop_ends_when_no_pair_is_left(tr, chunked):
    data = np.frombuffer(b"abcabdabcabd" * 40 + b"xyz", dtype=np.uint8)
    off = np.array([0, 100, 233, 301, len(data)], dtype=np.uint64) if chunked else None
    vocab = 256 + 3000
    want_m, want_c = O.train(data, vocab, off, mode=O.FIRST)
    assert 5 < len(want_m) < 40
    tr.set_option("first_wide", 1)
    tr.set_option("wide_from", 3)
    tr.set_option("conflict_resolution", 0)
    try:
        tr.load_corpus(data, off)
        tr.train_begin(vocab)
        done = tr.train_steps(vocab - 256)
        m, c = tr.train_result()
        st = tr.stats()
        assert tr.train_steps(10) == 0          # (and it stays ended)
    finally:
        _reset(tr)
    assert done == len(want_m) < vocab - 256
    assert m.tolist() == want_m.tolist() and c.tolist() == want_c.tolist()
    assert st["n_merges"] == len(want_m)
    assert int(c.min()) > 0


def test_first_no_pair_left_before_the_hand_over(tr):
    # small.txt, basic, vocabulary 70,000: the 16-bit part ends after 7 merges, nothing is converted
    data = read_data("small.txt")
    want = [[98, 99], [256, 100], [257, 101], [258, 258], [97, 259], [260, 258], [261, 10]]
    tr.set_option("first_wide", 1)
    try:
        m, c, st = tr.train(data, 70000, conflict_resolution=0)
    finally:
        _reset(tr)
    assert m.tolist() == want and st["n_merges"] == 7
    assert O.train(data, 70000, mode=O.FIRST)[0].tolist() == want


# ---- 4. real ids past 65,535, by exact recount -------------------------------------------------------------------

def _recount(toks, ends):
    """Exact overlapping-window counts of the live stream (no pair across a chunk end): (keys, counts, position keys)."""
    toks = toks.astype(np.uint64)
    n = len(toks)
    if n < 2:
        return np.zeros(0, np.uint64), np.zeros(0, np.int64), np.zeros(0, np.uint64)
    pkey = (toks[:-1] << np.uint64(32)) | toks[1:]
    pkey = np.where(ends[:-1] == 0, pkey, np.uint64(~np.uint64(0)))
    valid = pkey[pkey != ~np.uint64(0)]
    keys, counts = np.unique(valid, return_counts=True)
    return keys, counts, pkey


_RECOUNT = {}


def _recount_training(tr, chunked):
    """`first` training of test_ids_beyond_16_bits_real_counts_chunked's corpus at vocabulary 68,000 through the
    step-level API; at checkpoints the table equals a recount of the stream and the next merge is the recount's
    maximum, earliest first occurrence among the tied.  Returns (merges, counts, ties seen, non-lexical ties)."""
    if chunked in _RECOUNT:
        return _RECOUNT[chunked]
    data, off = _word_corpus(78, 4200, 24, (6, 14))
    if not chunked:
        off = None
    vocab = 68000
    n16 = (65518 if chunked else 65534) - 256         # (MBPE_MAX_VOCAB_CHUNKED / _BASIC: where the hand-over comes)
    cps = sorted({20000, n16 - 1, n16, n16 + 1, n16 + 40, 65535 - 256, n16 + 500, n16 + 1000, n16 + 1600, n16 + 2300})
    ties = non_lex = 0
    tr.set_option("conflict_resolution", 0)
    tr.set_option("first_wide", 1)
    try:
        tr.load_corpus(data, off)
        tr.train_begin(vocab)
        k = 0
        for cp in cps:
            assert tr.train_steps(cp - k) == cp - k
            toks, ends = tr.stream()
            if off is None:
                ends = np.zeros(len(toks), np.uint8)
                ends[-1:] = 1
            keys, counts, pkey = _recount(toks, ends)
            got = {kk: v for kk, v in tr.pairs_dict().items() if v}
            want = {(int(kk >> np.uint64(32)), int(kk & np.uint64(0xFFFFFFFF))): int(v) for kk, v in zip(keys, counts)}
            assert got == want, "pair table differs from the recount after %d merges" % cp
            M = int(counts.max())
            tied = keys[counts == M]
            at = int(np.flatnonzero(np.isin(pkey, tied))[0])
            a, b = int(toks[at]), int(toks[at + 1])
            assert tr.train_steps(1) == 1
            m, c = tr.train_result()
            assert (int(m[cp][0]), int(m[cp][1]), int(c[cp])) == (a, b, M), "merge %d" % cp
            if len(tied) > 1:
                ties += 1
                if int(tied.min()) != (a << 32 | b):
                    non_lex += 1
            k = cp + 1
        assert tr.train_steps(vocab) == vocab - 256 - k
        m, c = tr.train_result()
        import torch
        from mbpe import check
        dev = torch.device("cuda", 0)
        rt = check.decode_roundtrip(tr, m, torch.from_numpy(np.ascontiguousarray(data)).to(dev), torch, dev)
        assert rt["ok"], rt
    finally:
        _reset(tr)
    _RECOUNT[chunked] = (m, c, ties, non_lex)
    return _RECOUNT[chunked]


@pytest.mark.parametrize("chunked", [True, False])
def test_first_ids_beyond_16_bits_by_recount(tr, chunked):
    m, c, ties, non_lex = _recount_training(tr, chunked)
    assert len(m) == 68000 - 256
    assert ties >= 5 and non_lex >= 1
    assert int(c[65535 - 256]) >= 2 and int(c[65535 - 256 + 500]) >= 2 and int(m.max()) > 65535


# ---- 5. a tie beyond token 2^32 -------------------------------------------------------------------------------------

def test_first_wide_tie_beyond_token_2_pow_32():
    # test_first_mode_tie_beyond_slot_2_pow_32 with the hand-over at once: the 32-bit loop makes the choice
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda", 0)
    n = 5 << 30
    A, B, C, D = 65, 66, 67, 68
    buf = torch.empty(n + 16, dtype=torch.uint8, device=dev)
    step = 1 << 28
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    for lo in range(0, n, step):
        v = torch.randint(0, 252, (min(step, n - lo),), dtype=torch.int16, device=dev, generator=g)
        v = v + (v >= A).to(torch.int16) * 4                   # the filler never holds A, B, C or D
        buf[lo:lo + len(v)] = v.to(torch.uint8)
        del v
    tail = buf[4 << 30:n].view(-1, 2048)
    tail[:, 0], tail[:, 1] = C, D
    tail[:, 1024], tail[:, 1025] = A, B
    torch.cuda.synchronize()
    k = tail.shape[0]
    for mode, first_pair in ((0, [C, D]), (1, [A, B])):
        with mbpe.Trainer(0) as tr:
            tr.set_option("conflict_resolution", mode)
            tr.set_option("first_wide", 1)
            tr.set_option("wide_from", 0)
            tr.load_corpus_device(buf.data_ptr(), n, keep=buf)
            tr.train_begin(256 + 2)
            assert tr.train_steps(2) == 2
            m, c = tr.train_result()
            assert tr.stream_device()[2] == 32           # (the 32-bit loop made both merges)
        assert c.tolist() == [k, k], (mode, c.tolist())
        assert m[0].tolist() == first_pair and sorted(m.tolist()) == [[A, B], [C, D]], (mode, m.tolist())


# ---- 6. the CLI's default command line --------------------------------------------------------------------------

def _run(*args):
    r = subprocess.run([CLI] + [str(a) for a in args], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_cli_default_vocab_100000(tmp_path):
    # `minbpe-cc -t -i taylorswift.txt --vocab-size 100000`: gpt4 and `first` by default; no pair is left after
    # 10,161 merges, before the 32-bit loop would start
    model, enc, dec = tmp_path / "m", tmp_path / "enc", tmp_path / "dec"
    src = os.path.join(DATA, "taylorswift.txt")
    out = _run("-t", "-i", src, "-m", model, "--vocab-size", 100000)
    assert "Writing model..." in out
    data = read_data("taylorswift.txt")
    want_m, _ = O.train(data, 100000, mbpe.presplit(O.GPT4_SPLIT_PATTERN, data), mode=O.FIRST)
    assert len(want_m) == 10161
    assert model.read_bytes() == O.model_bytes(O.GPT4_SPLIT_PATTERN, want_m)
    _run("-e", "-i", src, "-m", model, "-o", enc)
    _run("-d", "-i", enc, "-m", model, "-o", dec)
    assert dec.read_bytes() == data


def test_cli_first_through_the_32_bit_loop(tr, tmp_path):
    # test 4's corpus as one chunk through the CLI: its model is the one of the merges checked by recount
    data, _ = _word_corpus(78, 4200, 24, (6, 14))
    src, model = tmp_path / "words.bin", tmp_path / "m"
    src.write_bytes(data.tobytes())
    _run("-t", "-i", src, "-m", model, "--encoder", "basic", "--vocab-size", 68000)
    m, _, _, _ = _recount_training(tr, False)
    assert len(m) == 68000 - 256 and int(m.max()) > 65535
    assert model.read_bytes() == O.model_bytes(O.PATTERNS["basic"], m)


def test_first_small_txt_cli_vocab_70000(tmp_path):
    model = tmp_path / "m"
    _run("-t", "-i", os.path.join(DATA, "small.txt"), "-m", model, "--encoder", "basic", "--vocab-size", 70000)
    lines = model.read_bytes().decode("utf-8").split("\n")
    assert lines[3 + int(lines[2]):][:-1] == ["98 99", "256 100", "257 101", "258 258", "97 259", "260 258", "261 10"]


# ---- 7. opt-in stays opt-in -------------------------------------------------------------------------------------

def test_first_beyond_16_bits_without_the_option(tr):
    data = b"hello world hello world"
    tr.set_option("conflict_resolution", 0)
    try:
        tr.load_corpus(data)
        with pytest.raises(mbpe.MbpeError) as e:
            tr.train_begin(65535)
        assert e.value.code == mbpe.ERR_VOCAB
        tr.load_corpus(data, np.array([0, 6, len(data)], dtype=np.uint64))
        with pytest.raises(mbpe.MbpeError) as e:
            tr.train_begin(65519)
        assert e.value.code == mbpe.ERR_VOCAB
        with pytest.raises(mbpe.MbpeError) as e:
            tr.train(data, 65535, conflict_resolution=0)        # (mbpe_train does not force the option)
        assert e.value.code == mbpe.ERR_VOCAB
    finally:
        _reset(tr)
