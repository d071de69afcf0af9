"""What a training leaves behind for the next one on the same Trainer: six trainings in a row that take every route of
the begin (csrc/train_plan.h) -- the slot stream, the conversion to the 32-bit loop (csrc/wide_run.cpp), the direct
begin of a weighted corpus, the same under a length limit, the direct begin of a continued training, and the slot stream
again -- each against the oracle; the last one must equal the first bit for bit, and the context must then report a
slot stream.  One more case makes the 32-bit loop grow its pair table between two groups of merges."""
import numpy as np
import pytest

import mbpe
import oracle as O
import dedup_cases as C

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

VOCAB = 320
SLOT_FIGURES = ("n_slots", "n_live", "n_merges", "n_pairs", "n_batches")


def _limited_first(data, off, vocab, max_len):
    """The `first` tie-break under "max_token_length" (mbpe.h), decided on the oracle's table and stream: the largest
    count among the pairs whose halves are at most max_len bytes together, the earliest first occurrence among its ties;
    the training ends when no pair is eligible or that count is 0."""
    st = O.State(data, off, O.FIRST)
    length = [1] * 256
    merges, counts = [], []
    while len(merges) < vocab - 256:
        ok = {p: c for p, c in st.table_dict().items() if c > 0 and length[p[0]] + length[p[1]] <= max_len}
        if not ok:
            break
        top = max(ok.values())
        ties = [p for p, c in ok.items() if c == top]
        if len(ties) > 1:
            toks, clen = st.stream()
            keys = (toks[:-1].astype(np.uint64) << np.uint64(32)) | toks[1:].astype(np.uint64)
            inside = np.ones(len(keys), dtype=bool)
            inside[np.cumsum(clen[clen > 0]).astype(np.int64)[:-1] - 1] = False      # (no pair across a chunk end)
            hit = np.isin(keys, np.array([(a << 32) | b for a, b in ties], dtype=np.uint64)) & inside
            at = int(np.argmax(hit))
            ties = [(int(toks[at]), int(toks[at + 1]))]
        a, b = ties[0]
        st.merge(a, b, 256 + len(merges))
        length.append(length[a] + length[b])
        merges.append([a, b])
        counts.append(top)
    st.close()
    return merges, counts


def test_six_trainings_on_one_trainer():
    data = O.splitmix64_bytes(31, 16 << 10)
    data[data == 0] = 1                                  # (no chunk the NUL rule could make inert)
    off = np.array(list(range(0, len(data), 7)) + [len(data)], dtype=np.uint64)
    want_m, want_c = O.train(data, VOCAB, off, O.LEXICAL)
    assert len(want_m) == VOCAB - 256 and int(want_c[-1]) >= 1
    rng = np.random.default_rng(5)
    uniq = list(dict.fromkeys(bytes(x) for x in rng.integers(97, 101, size=(600, 8), dtype=np.uint8)))[:512]
    assert len(uniq) == 512
    weights = np.arange(1, 513, dtype=np.uint32)
    u_data, u_off = C.join(uniq)
    f_data, f_off = C.join([c for c, w in zip(uniq, weights.tolist()) for _ in range(w)])
    want3_m, want3_c = O.train(f_data, VOCAB, f_off, O.FIRST)
    want4_m, want4_c = _limited_first(f_data, f_off, VOCAB, 4)
    assert 0 < len(want4_m) <= VOCAB - 256 and want4_m != want3_m.tolist()      # (the limit bites)

    def run(tr, prior=None):
        tr.train_begin(VOCAB, prior)
        tr.train_steps(VOCAB - 256)
        return tr.train_result()

    with mbpe.Trainer(0) as tr:
        # 1. the slot stream
        tr.load_corpus(data, off)
        m1, c1 = run(tr)
        assert m1.tolist() == want_m.tolist() and c1.tolist() == want_c.tolist()
        st1, toks1 = tr.stats(), tr.stream()
        assert tr.stream_device()[2] == 16
        # 2. the same corpus, handed over to the 32-bit loop after 8 merges
        tr.set_option("wide_from", 8)
        m, c = run(tr)
        assert m.tolist() == want_m.tolist() and c.tolist() == want_c.tolist()
        assert tr.stream_device()[2] == 32 and tr.stats()["n_slots"] == tr.stats()["n_live"] == len(toks1[0])
        tr.set_option("wide_from", -1)
        # 3. distinct chunks with weights, `first`: 32-bit tokens from the first merge
        tr.load_corpus_weighted(u_data, u_off, weights)
        tr.set_option("conflict_resolution", 0)
        m, c = run(tr)
        assert m.tolist() == want3_m.tolist() and c.tolist() == want3_c.tolist()
        # 4. the same under a length limit
        tr.set_option("max_token_length", 4)
        m, c = run(tr)
        assert m.tolist() == want4_m and c.tolist() == want4_c
        tr.set_option("max_token_length", 0)
        tr.set_option("conflict_resolution", 1)
        # 5. continued from the first 16 merges of training 1 on its corpus, directly on 32-bit tokens
        tr.load_corpus(data, off)
        tr.set_option("resume_wide", 1)
        tr.set_option("wide_from", 0)
        m, c = run(tr, m1[:16])
        assert m.tolist() == want_m.tolist()
        assert c[:16].tolist() == [-1] * 16 and c[16:].tolist() == want_c[16:].tolist()
        assert tr.stream_device()[2] == 32
        tr.set_option("resume_wide", 0)
        tr.set_option("wide_from", -1)
        # 6. training 1 again: the same result bit for bit, and the slot stream's figures, not a 32-bit stream's
        m6, c6 = run(tr)
        assert m6.tobytes() == m1.tobytes() and c6.tobytes() == c1.tobytes()
        st6, toks6 = tr.stats(), tr.stream()
        assert tr.stream_device()[2] == 16
        assert {k: st6[k] for k in SLOT_FIGURES} == {k: st1[k] for k in SLOT_FIGURES}
        assert st6["n_live"] == len(toks6[0])
        assert np.array_equal(toks6[0], toks1[0]) and np.array_equal(toks6[1], toks1[1])


def test_the_32_bit_loop_grows_its_table():
    """600 merges on 16 KiB of random bytes in one chunk, all of them in the 32-bit loop.  The commit before the loop's host
    code became csrc/wide_run.cpp reported n_table_grows = 1 on this input at 600 merges, measured on an MI355X; so does
    this one."""
    data = O.splitmix64_bytes(32, 16 << 10)
    data[data == 0] = 1
    vocab = 256 + 600
    want_m, want_c = O.train(data, vocab, None, O.LEXICAL)
    with mbpe.Trainer(0) as tr:
        tr.load_corpus(data)
        tr.set_option("wide_from", 0)
        tr.train_begin(vocab)
        assert tr.train_steps(vocab - 256) == vocab - 256
        m, c = tr.train_result()
        grows = tr.stats()["n_table_grows"]
    print("n_table_grows", grows)
    assert m.tolist() == want_m.tolist() and c.tolist() == want_c.tolist()
    assert grows >= 1
