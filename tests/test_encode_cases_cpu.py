"""The oracle's encode against a second reference on the shapes of tests/encode_cases.py.

tests/test_gpu_encode_spans.py judges the device encode by `oracle.encode_chunks` (bpe_oracle.c) on inputs of megabytes.
Here the same generators run at 1/32 of the kernels' geometry (spans of 32 tokens, 32 slices: the same per values, the
same positions relative to span and slice edges, at most 64 Ki bytes) and the oracle must equal the brute-force encode
of tests/test_bruteforce_cpu.py -- Python lists, a dict, `text_to_vector` restated from the reference with a regular
expression -- chunk by chunk.  The generators' own promises (span counts, wrapping chains) are asserted too."""
import numpy as np
import pytest

import encode_cases as E
import oracle as O
from test_bruteforce_cpu import brute_force_encode_chunk, brute_force_encode_passes, text_to_vector

SCALE = 1 / 32


def brute_force_chunks(case):
    """-> (tokens of all chunks, 1 + the largest number of replacing passes of a chunk; 0 for an empty text)"""
    lookup = {(int(a), int(b)): 256 + k for k, (a, b) in enumerate(case.merges.tolist())}
    data = case.data.tobytes()
    off = [0, len(data)] if case.chunk_off is None else [int(o) for o in case.chunk_off]
    out, deepest = [], 0
    for s, e in zip(off[:-1], off[1:]):
        toks, replacing = brute_force_encode_passes(text_to_vector(data[s:e]), lookup)
        out += toks
        deepest = max(deepest, replacing)
    return np.array(out, dtype=np.uint32), (1 + deepest if len(data) else 0)


def _agree(case):
    assert len(case.data) <= 64 << 10, case.name
    want, _ = brute_force_chunks(case)
    got = O.encode_chunks(case.data, case.chunk_off, case.merges)
    assert np.array_equal(got, want), case.name


def test_text_to_vector_quirks():
    # Tokenizer.h:86-93 with std::stoi's rules
    assert text_to_vector(b"\x0012abc") == [12] and text_to_vector(b"\x00 12") == [12] and text_to_vector(b"\x00+7") == [7]
    assert text_to_vector(b"\x00 \t\n\v\f\r7") == [7] and text_to_vector(b"\x00-0") == [0]
    assert text_to_vector(b"\x00abc") == [0, 97, 98, 99] and text_to_vector(b"\x00") == [0]
    assert text_to_vector(b"\x00\x0012") == [0, 0, 49, 50] and text_to_vector(b"\x007\x0012") == [7]
    assert text_to_vector(b"\x002147483647") == [2147483647]
    assert text_to_vector(b"\x002147483648") == list(b"\x002147483648")
    assert text_to_vector(b"\x00" + b"9" * 20) == [0] + [57] * 20
    assert text_to_vector(b"\x00-1") == [0xFFFFFFFF] and text_to_vector(b"\x00-2147483648") == [0x80000000]
    assert text_to_vector(b"\x00+-7") == [0, 43, 45, 55] and text_to_vector(b"12") == [49, 50]
    # the two encode loops of test_bruteforce_cpu.py (one is the other plus a counter)
    lookup = {(49, 50): 256, (256, 256): 257}
    toks = [49, 50] * 5
    assert brute_force_encode_passes(toks, lookup) == (brute_force_encode_chunk(toks, lookup), 2)
    assert brute_force_encode_passes([7], lookup) == ([7], 0)


def test_run_cases_have_the_spans_they_promise():
    for scale in (SCALE, 1.0):
        span, slices, _ = E.geometry(scale)
        cases = E.run_cases(scale)
        assert sorted(set(-(-len(c.data) // span) for c in cases)) == \
            [slices - 1, slices, slices + 1, 2 * slices - 1, 2 * slices, 2 * slices + 1, 3 * slices + 1, 5 * slices + 1]
        assert sorted(set(-(-len(c.data) // (span * slices)) for c in cases)) == [1, 2, 3, 4, 6]
        seen = set()
        for c in cases:
            if c.chunk_off is not None:
                per = -(-len(c.data) // (span * slices))
                d = [((int(o) + 1) % (span * per)) - 1 for o in c.chunk_off[1:-1]]
                assert d and set(d) <= {-1, 0, 1}, c.name
                seen |= set((per, v) for v in d)
        assert seen == set((per, v) for per in (1, 2, 3, 4, 6) for v in (-1, 0, 1))


@pytest.mark.parametrize("index", range(96))
def test_oracle_equals_brute_force_on_run_cases(index):
    _agree(E.run_cases(SCALE)[index])


@pytest.mark.parametrize("seed", range(4))
def test_oracle_equals_brute_force_on_fuzz_cases(seed):
    _agree(E.fuzz_case(np.random.default_rng(4200 + seed), SCALE / 4))


def test_oracle_equals_brute_force_on_nul_cases():
    cases = E.nul_cases(np.random.default_rng(4300), SCALE)
    for c in cases:
        _agree(c)
    for c in E.nul_error_cases():              # (a token on the host: both references agree on it)
        _agree(c)
    # at least one NUL-led chunk of more than 64 bytes
    assert any(int(e) - int(s) > 64 and c.data[int(s)] == 0 for c in cases
               for s, e in zip(c.chunk_off[:-1], c.chunk_off[1:]))


def test_nul_cases_straddle_the_edges_they_name():
    for scale in (SCALE, 1.0):
        span, slices, group = E.geometry(scale)
        cases = E.nul_cases(np.random.default_rng(4300), scale)
        straddled = set()
        for c in cases:
            per = -(-len(c.data) // (span * slices))
            units = [(group, "group"), (span, "span")] + ([(span * per, "slice")] if per > 1 else [])
            for s, e in zip(c.chunk_off[:-1], c.chunk_off[1:]):
                s, e = int(s), int(e)
                if c.data[s] == 0:
                    straddled |= set(tag for unit, tag in units if (e - 1) // unit > s // unit)
            assert c.data[0] == 0 and c.data[int(c.chunk_off[-2])] == 0, c.name          # first and last chunk
        assert straddled == {"group", "span", "slice"}
        assert sum(c.tok is not None for c in cases) >= 2


def test_oracle_equals_brute_force_on_lookup_cases():
    cases = E.lookup_cases(SCALE / 2)
    assert [len(c.merges) for c in cases] == [1, 7, 8, (1 << 15) - 1, 1 << 15, 100000, 50]
    for c in cases:
        _agree(c)
        if len(c.merges) != 50:                                     # the last merge of the table occurs
            assert int(O.encode_chunks(c.data, c.chunk_off, c.merges).max()) == 256 + len(c.merges) - 1, c.name
    assert int(cases[5].merges[-1].min()) > 65535                   # sides beyond 16 bits that a text produces


def test_lookup_case_has_a_chain_that_wraps_the_table_end():
    # E.enc_hash mirrors pair_hash() of csrc/span.h; E.table_bits and E.build_table mirror the capacity rule
    # (`while ((1ull << bits) < 2ull * n_merges + 2) ++bits;`) and the insertion loop of encode_chunks() there
    case = E.lookup_cases(SCALE)[-1]
    slots, bits = E.build_table(case.merges.tolist())
    cap = 1 << bits
    assert cap == 128 and sum(k is not None for k in slots) == len(case.merges)
    homes, length = E.tail_chain(slots, bits)
    wrapped = E.wrapped_keys(slots, bits)
    assert len(homes) >= 4 and len(wrapped) >= 4 and length >= 6 and slots[0] is not None
    # the text looks up pairs that are stored behind the wrap, and absent pairs whose probe starts in that chain
    pass1 = O.encode_chunks(case.data, None, case.merges[:36])
    pairs = set((int(a) << 32) | int(b) for a, b in zip(pass1[:-1], pass1[1:]))
    present = set(k for k in slots if k is not None)
    assert pairs & set(wrapped)
    assert any(k not in present and E.enc_hash(k, 64 - bits) >= cap - 2 for k in pairs)
