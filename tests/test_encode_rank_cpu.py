"""Rank-ordered encode on the CPU: the three restatements of tests/encode_rank_cases.py against each other, and the
host loop of Tokenizer.encode(order="rank") against them on every golden model.

(a) the min-id loop equals the in-order replay on every well-formed case (the literal per-chunk loop, the replay, and
    the numpy loop over all chunks that judges the GPU tests; the generators run at 1/32 of the kernels' geometry)
(b) the host Tokenizer equals the reference for every golden .model with its data file, special tokens included
(c) the default order is still the reference's greedy passes
(d) the two orders differ: the three-byte witness, and taylorswift.txt with its gpt4 model
(e) a repeated pair and a merge side at or above its own id follow the loop, not the replay"""
import json
import os

import numpy as np
import pytest

import mbpe
import oracle as O
import encode_rank_cases as R
from conftest import GOLDEN, read_data, read_golden
from test_bruteforce_cpu import brute_force_encode_chunk, text_to_vector

INDEX = json.load(open(os.path.join(GOLDEN, "index.json")))
SCALE = 1 / 32


def _small_cases():
    out = [R.placement_case(SCALE)] + R.run_cases(SCALE) + R.slice_cases(SCALE) + [R.special_case(SCALE)]
    out += [R.fuzz_case(200 + s, n_bytes=6000, max_merges=300) for s in range(4)]
    return out


def test_loop_equals_replay_on_every_well_formed_case():
    cases = _small_cases()
    assert len(cases) == 1 + 48 + 3 + 1 + 4
    for c in cases:
        # (the table of the special-token case has special ids as sides: there the loop alone is the definition)
        assert R.well_formed(c.merges) == (not c.name.startswith("specials")), c.name
        want, want_off, passes = R.rank_loop_chunks(c.data, c.chunk_off, c.merges)
        tok, end, pass_tokens = R.reference(c)
        assert np.array_equal(tok, want) and len(pass_tokens) == passes, c.name
        assert np.array_equal(R.chunk_tok_off(end, len(c.data), c.chunk_off), want_off), c.name
        stream = R.token_stream(c.data, c.chunk_off)
        assert pass_tokens[0] == len(stream[0])
        if not R.well_formed(c.merges):
            continue
        assert np.array_equal(R.replay_chunks(c.data, c.chunk_off, c.merges), want), c.name
        replayed = R.replay_text(*stream, c.merges)
        assert np.array_equal(replayed[0], want) and np.array_equal(replayed[1], end), c.name


def test_singles_are_the_nul_led_chunks_by_position():
    a, b = R.special_case(SCALE), R.special_case(SCALE, as_singles=True)
    assert b.singles and not np.array_equal(a.data, b.data)
    assert np.array_equal(R.reference(a)[0], R.reference(b)[0])


def _golden(name):
    meta = INDEX[name]
    pattern, _, merges = O.parse_model(read_golden(name + ".model"))
    assert pattern == O.PATTERNS[meta["encoder"]]
    return pattern, merges


def _data_of(name):
    if name.startswith("splitmix42"):
        return O.splitmix64_bytes(42, 1 << 14).tobytes()                 # (one chunk: a round per merge that applies)
    data = read_data(name.split("_")[0] + ".txt")
    return data if "gpt" in name else data[:100000]


@pytest.mark.parametrize("name", sorted(INDEX))
def test_host_tokenizer_equals_the_reference_on_the_golden_models(name):
    pattern, merges = _golden(name)
    assert R.well_formed(merges)
    data = _data_of(name)
    off = mbpe.presplit(pattern, np.frombuffer(data, dtype=np.uint8)) if pattern else None
    stream = R.token_stream(data, off)
    want = R.rank_loop_text(*stream, merges)[0]
    assert np.array_equal(R.replay_text(*stream, merges)[0], want)
    tok = mbpe.Tokenizer(pattern)
    tok.set_merges(merges)
    got = tok.encode(data, order="rank")
    assert np.array_equal(got, want)
    assert tok.decode(got) == data
    greedy = tok.encode(data)                                         # (c) the default, and the order is per call
    assert np.array_equal(greedy, tok.encode(data, order="greedy"))
    assert np.array_equal(greedy, O.encode_chunks(data, off, merges))
    tok.close()


def _special_chunks(tok_pattern, text, specials):
    """split_on_special (earliest occurrence of any name), then the pattern's chunks of every other part; a special
    token travels as the chunk NUL + decimal id -> (buffer, chunk offsets)"""
    parts, pos = [], 0
    while True:
        hits = [(text.find(n, pos), n) for n in specials if text.find(n, pos) >= 0]
        if not hits:
            parts.append(text[pos:])
            break
        at, name = min(hits)
        parts += [text[pos:at], b"\0%d" % specials[name]]
        pos = at + len(name)
    buf, off = b"", [0]
    for p in parts:
        if not p:
            continue
        if p[:1] == b"\0":
            cuts = [len(p)]
        else:
            cuts = mbpe.presplit(tok_pattern, np.frombuffer(p, dtype=np.uint8))[1:].tolist()
        off += [len(buf) + c for c in cuts]
        buf += p
    return buf, np.array(off, dtype=np.uint64)


def test_host_tokenizer_with_special_tokens():
    pattern, merges = _golden("taylorswift_gpt4_first_512")
    specials = {}
    for ln in read_data("special1.txt").decode().split("\n"):
        if ln.strip():
            name, idx = ln.rsplit(" ", 1)
            specials[name.encode()] = int(idx)
    text = read_data("specialtokensample.txt")
    buf, off = _special_chunks(pattern, text, specials)
    want, _, _ = R.rank_loop_chunks(buf, off, merges)
    assert set(specials.values()) & set(want.tolist())
    tok = mbpe.Tokenizer(pattern)
    tok.set_special_tokens_from_file(read_data("special1.txt"))
    tok.set_merges(merges)
    got = tok.encode(text, order="rank")
    assert got.tolist() == want.tolist()
    assert tok.decode(got) == text
    # (c) the default with special tokens: the brute-force greedy loop chunk by chunk
    lookup = R.lookup_of(merges)
    greedy = sum((brute_force_encode_chunk(text_to_vector(c), lookup) for c in R.chunks_of(buf, off)), [])
    assert tok.encode(text).tolist() == greedy
    with pytest.raises(ValueError):
        tok.encode(text, order="first")
    with pytest.raises(ValueError):
        tok.encode(text, order=1)
    tok.close()


def test_the_two_orders_differ():
    # merges [(b,c), (a,b)], text abc: greedy takes (a,b) first because it comes first in the text
    merges = np.array([[98, 99], [97, 98]], dtype=np.uint32)
    lookup = R.lookup_of(merges)
    assert brute_force_encode_chunk([97, 98, 99], lookup) == [257, 99]
    assert R.rank_loop_chunk([97, 98, 99], lookup) == ([97, 256], 1)
    assert R.replay_chunk([97, 98, 99], merges) == [97, 256]
    tok = mbpe.Tokenizer("")
    tok.set_merges(merges)
    assert tok.encode(b"abc").tolist() == [257, 99]
    assert tok.encode(b"abc", order="rank").tolist() == [97, 256]
    assert tok.encode(b"abc").tolist() == [257, 99]                   # the order does not stick
    tok.close()
    # a a a with (a,a): m a
    assert R.rank_loop_chunk([97, 97, 97], {(97, 97): 256}) == ([256, 97], 1)
    pattern, merges = _golden("taylorswift_gpt4_lexical_512")
    data = read_data("taylorswift.txt")
    tok = mbpe.Tokenizer(pattern)
    tok.set_merges(merges)
    greedy, rank = tok.encode(data), tok.encode(data, order="rank")
    assert not np.array_equal(greedy, rank)
    assert tok.decode(greedy) == tok.decode(rank) == data
    tok.close()


def test_tables_that_are_not_well_formed_follow_the_loop():
    tok = mbpe.Tokenizer("")
    # a repeated pair keeps the last id: (a,b) is 258, so (b,c) = 257 goes first; the replay would take (a,b) as 256
    assert not R.well_formed(R.REPEATED_PAIR)
    lookup = R.lookup_of(R.REPEATED_PAIR)
    assert lookup == {(97, 98): 258, (98, 99): 257}
    assert R.rank_loop_chunk(list(b"abcab"), lookup) == ([97, 257, 258], 2)
    assert R.replay_chunk(list(b"abcab"), R.REPEATED_PAIR) == [256, 99, 256]
    tok.set_merges(R.REPEATED_PAIR)
    assert tok.encode(b"abcab", order="rank").tolist() == [97, 257, 258]
    assert np.array_equal(R.rank_loop_text(*R.token_stream(b"abcab", None), R.REPEATED_PAIR)[0], [97, 257, 258])
    # merge 0 = (257, c) needs the token merge 1 makes: the loop reaches it in its second round, the replay never
    assert not R.well_formed(R.HIGH_SIDE)
    lookup = R.lookup_of(R.HIGH_SIDE)
    assert R.rank_loop_chunk(list(b"abcab"), lookup) == ([256, 257], 2)
    assert R.replay_chunk(list(b"abcab"), R.HIGH_SIDE) == [257, 99, 257]
    tok.set_merges(R.HIGH_SIDE)
    assert tok.encode(b"abcab", order="rank").tolist() == [256, 257]
    assert np.array_equal(R.rank_loop_text(*R.token_stream(b"abcab", None), R.HIGH_SIDE)[0], [256, 257])
    tok.close()
