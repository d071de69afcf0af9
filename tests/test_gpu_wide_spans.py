"""The 32-bit merge loop (csrc/wide.hip) on more than 1,024 spans.

Its passes cut the token stream into spans of kSpan = 1,024 tokens (csrc/span.h) and link them with two single-workgroup scans
of 1,024 threads (k_wide_scan_parity, k_wide_scan_sum), thread t owning per = ceil(n_spans / 1,024) consecutive spans.
tests/test_gpu_wide.py stays below 21 spans (per = 1) and the 5 GiB case of tests/test_gpu_wide_first.py has no span
whose every position is a candidate.  Here: runs and `ab` / `aab` periods of megabytes (full spans, per = 6),
chunk ends at the slice edges, the conversion k_wide_from_slots on a slot stream with barrier slots (its holes), and the
hand-over fuzz at its full sizes -- with the step-parity helpers of the existing files: chosen pair, count, whole
stream, chunk ends and pair table against the oracle after every merge."""
import numpy as np
import pytest

import mbpe
import oracle as O
import encode_cases as E
from conftest import read_data
from test_gpu_parity import _defaults, _step_parity
from test_gpu_wide_first import _first_step_parity

pytestmark = pytest.mark.gpu

N = 6 << 20
VOCAB = 256 + 12


@pytest.fixture(scope="module")
def tr():
    t = mbpe.Trainer(0)
    yield t
    t.close()


def _corpus():
    """A run, an `ab` period and an `aab` period of N / 3 bytes each: N = 6 Mi tokens, 6 spans per scan thread.  One
    other byte first: the run starts at an odd position, so the spans behind the first -- all of them full -- hand an
    odd parity on from slice to slice (from position 0 every parity of the one-chunk case would be even)."""
    third = N // 3
    return np.frombuffer(b"z" + b"a" * third + b"ab" * (third // 2) + b"aab" * (third // 3), dtype=np.uint8)


def _cuts(n):
    """Chunk ends at k * 1,024 * per + {-1, 0, +1} for the first, a middle and the last slice of the first pass."""
    cuts = sorted(set(c for rot in range(3) for c in E.slice_edge_cuts(n, E.SPAN, E.SLICES, rot)))
    per = -(-n // (E.SPAN * E.SLICES))
    assert per >= 2 and len(cuts) == 9 and all(((c + 1) % (E.SPAN * per)) - 1 in (-1, 0, 1) for c in cuts)
    return np.array([0] + cuts + [n], dtype=np.uint64)


def _spans_after(data, off, merges):
    st = O.State(data, off)
    out = []
    for i, (a, b) in enumerate(merges):
        out.append(-(-len(st.stream()[0]) // E.SPAN))
        st.merge(int(a), int(b), 256 + i)
    st.close()
    return out


def test_the_first_merges_run_on_more_than_1024_spans():
    # (a property of the corpus, from the oracle: the first three merges of either tie-break read > 1,024 spans)
    data = _corpus()
    for mode in (O.LEXICAL, O.FIRST):
        m, _ = O.train(data, 256 + 3, None, mode=mode)
        assert all(s > E.SLICES for s in _spans_after(data, None, m)), mode


@pytest.mark.parametrize("chunked", [False, True], ids=["one_chunk", "cuts_at_slice_edges"])
@pytest.mark.parametrize("mode", ["lexical", "first"])
def test_step_parity_runs_on_many_spans_wide(tr, mode, chunked):
    data = _corpus()
    off = _cuts(len(data)) if chunked else None
    if mode == "lexical":
        _step_parity(tr, data, off, VOCAB, batch=1, wide_from=0)
    else:
        _first_step_parity(tr, data, off, VOCAB, 0, batch=1)


@pytest.mark.parametrize("mode", ["lexical", "first"])
def test_step_parity_hand_over_with_holes_on_many_spans(tr, mode):
    """Two merges on the 16-bit slot stream, no compaction on the way ("compact_den" 0), chunk ends as barrier slots:
    k_wide_from_slots reads more than 1,024 spans of slots, drops the barriers (wide_convert compacts the merges' holes
    away itself; the barriers are the holes that remain) and its sum scan places every span."""
    data = _corpus()
    # (5,000 chunks of 3,591 bytes next to the one-byte chunks at the slice edges: barrier slots in most spans)
    off = np.unique(np.concatenate([_cuts(len(data)), np.arange(1, 40000, 7, dtype=np.uint64) * np.uint64(513)]))
    off = off[off <= len(data)].astype(np.uint64)
    if mode == "lexical":
        _step_parity(tr, data, off, VOCAB, batch=1, wide_from=2, chunk_barrier=1, compact_den=0)
    else:
        _first_step_parity(tr, data, off, VOCAB, 2, batch=1, chunk_barrier=1, compact_den=0)


def _case_at(rng, text, n):
    """The kinds of corpus of test_gpu_fuzz._case at a given size."""
    kind = int(rng.integers(0, 5))
    if kind == 0:
        data = rng.integers(0, int(rng.choice([2, 3, 5, 17, 64, 256])), size=n, dtype=np.uint8)
    elif kind == 1:      # repeated blocks: many equal counts
        blk = rng.integers(97, 97 + int(rng.integers(2, 26)), size=int(rng.integers(3, 400)), dtype=np.uint8)
        data = np.tile(blk, n // len(blk) + 1)[:n]
    elif kind == 2:      # long runs: (t,t) merges
        vals = rng.integers(97, 101, size=max(n // 50, 1), dtype=np.uint8)
        data = np.repeat(vals, rng.integers(1, 100, size=len(vals)))[:n]
    elif kind == 3:      # a text slice repeated
        s = int(rng.integers(0, len(text) - 5000))
        l = int(rng.integers(50, 5000))
        data = np.frombuffer((text[s:s + l] * (n // l + 1))[:n], dtype=np.uint8).copy()
    else:                # NUL-heavy
        data = rng.integers(0, 4, size=n, dtype=np.uint8)
    data = np.ascontiguousarray(data)
    off = None
    if rng.integers(0, 3) == 0:
        cuts = np.unique(rng.integers(1, len(data), size=max(len(data) // int(rng.integers(2, 200)), 1)))
        off = np.concatenate([[0], cuts, [len(data)]]).astype(np.uint64)
    return kind, data, off


@pytest.mark.parametrize("seed", range(2))
def test_fuzz_wide_handover_at_full_size(tr, seed):
    """The hand-over fuzz of tests/test_gpu_fuzz.py without its truncation to 20,000 bytes: 1-4 MiB, lexical, the
    32-bit loop from a random merge on; merges, counts, final stream and pair table against the oracle."""
    text = read_data("shakespeare.txt")
    for case in range(3):
        rng = np.random.default_rng(9500 + seed * 100 + case)
        kind, data, off = _case_at(rng, text, int(rng.integers(1 << 20, (4 << 20) + 1)))
        vocab = 256 + int(rng.integers(10, 61))
        wf = int(rng.integers(0, vocab - 256 + 1))
        tag = (seed, case, kind, len(data), vocab, wf, off is not None)
        opts = {"compact_den": int(rng.choice([0, 2, 8])), "chunk_barrier": int(rng.choice([-1, 1])),
                "lockstep": int(rng.choice([0, 1])), "wide_from": wf}
        for k, v in opts.items():
            tr.set_option(k, v)
        try:
            want_m, want_c = O.train(data, vocab, off)
            m, c, _ = tr.train_lexical(data, vocab, off)
            assert m.tolist() == want_m.tolist() and c.tolist() == want_c.tolist(), tag
            st = O.State(data, off)
            for i, (a, b) in enumerate(want_m):
                st.merge(int(a), int(b), 256 + i)
            starts = np.array([0], dtype=np.int64) if off is None else off[:-1].astype(np.int64)
            if not np.any(data[starts] == 0):            # (a NUL-led chunk: same merges, different stream listing)
                assert np.array_equal(tr.stream()[0], st.stream()[0]), tag
            assert {k: v for k, v in tr.pairs_dict().items() if v} == \
                   {k: v for k, v in st.table_dict().items() if v}, tag
            st.close()
        finally:
            _defaults(tr)
