"""BPE-dropout on the CPU: the shared arithmetic of csrc/dropout.h as a stand-alone program (plain and under ASan +
UBSan), the Python restatement of the hash against the known answers and its drop fraction, the restatements of the
loop against each other, and the host loop of Tokenizer.encode(order="rank", dropout=p, seed=s) through the C-ABI
against the oracle of tests/dropout_cases.py.  No GPU."""
import math
import os
import subprocess

import numpy as np
import pytest

import mbpe
import oracle as O
import dropout_cases as D
import encode_rank_cases as R
from byteoff_cases import parse_special, vocab_bytes
from conftest import read_data, read_golden
from test_encode_rank_cpu import _special_chunks

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "minbpe-cc_amd", "csrc")

FLAGS = {
    "plain": ["-O2"],
    "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
}


@pytest.mark.parametrize("build", sorted(FLAGS))
def test_dropout_arithmetic(build, tmp_path):
    exe = str(tmp_path / "dropout_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Wextra", "-Werror"] + FLAGS[build] +
                          ["-I" + CSRC, os.path.join(HERE, "dropout_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.strip().endswith("ok: 400 strings, 0 failures")


def test_python_hash_equals_the_known_answers():
    for seed, pos, idx, want in D.KNOWN:
        assert D.drop_hash(seed, pos, idx) == want
        assert int(D.drop_hash_np(seed, np.array([pos], dtype=np.uint64), np.array([idx]))[0]) == want
    assert D.threshold_of(0.0) == 0 and D.threshold_of(1.0) == 1 << 32 and D.threshold_of(0.5) == 1 << 31
    assert D.threshold_of(2.0 ** -32) == 1 and D.threshold_of(0.1) == 429496729


def test_threshold_helper_of_the_library():
    for p in (0.0, 1.0, 0.5, 2.0 ** -32, 0.1, 0.25, 1.0 - 2.0 ** -40):
        assert mbpe.dropout_threshold(p) == D.threshold_of(p)
    for p in (-0.1, 1.0000001, 2.0, float("nan"), float("inf"), float("-inf")):
        with pytest.raises(mbpe.MbpeError) as e:
            mbpe.dropout_threshold(p)
        assert e.value.code == mbpe.ERR_ARG


@pytest.mark.parametrize("seed", [0, 1, 12345])
def test_drop_fraction(seed):
    n = 1 << 20
    pos = np.arange(n, dtype=np.uint64)
    for p in (0.1, 0.5):
        th = D.threshold_of(p)
        bound = 5 * math.sqrt(n * p * (1 - p))
        for idx in (256, 300):
            cnt = int((D.drop_hash_np(seed, pos, np.full(n, idx, dtype=np.uint64)) < th).sum())
            print(seed, p, idx, cnt, (cnt - n * p) / math.sqrt(n * p * (1 - p)))
            assert abs(cnt - n * p) <= bound, (seed, p, idx, cnt)
        cnt = int((D.drop_hash_np(seed, np.full(n, 77, dtype=np.uint64), 256 + pos) < th).sum())
        print(seed, p, "ids at pos 77", cnt, (cnt - n * p) / math.sqrt(n * p * (1 - p)))
        assert abs(cnt - n * p) <= bound, (seed, p, cnt)


def test_the_restatements_agree():
    strings, merges = D.generated_strings()
    lookup = R.lookup_of(merges)
    differing = 0
    for k, s in enumerate(strings):
        plain = R.rank_loop_chunk(list(s), lookup)[0] if s else []
        for th in (0, 1 << 30, 1 << 31, D.ONE):
            seed, base = (0, 1, 12345)[k % 3], (0, 1000, 1 << 40)[k % 3]
            tok, pos, _ = D.dropout_loop_chunk(list(s), lookup, base, seed, th)
            t2, e2, p2, _ = D.dropout_loop_text(np.array(list(s), dtype=np.uint32),
                                                np.arange(len(s)) == len(s) - 1,
                                                base + np.arange(len(s), dtype=np.uint64), merges, seed, th)
            assert tok == t2.tolist() and pos == p2.tolist(), (s, th)
            if th == 0:
                assert tok == plain
            if th == D.ONE:
                assert tok == list(s)
            differing += tok != plain
    assert differing > 100
    # a a a with (a,a): the instance at 0 dropped and the one at 1 not -> a m
    th = 1 << 31
    seed = next(s for s in range(64) if D.dropped(s, 0, 256, th) and not D.dropped(s, 1, 256, th))
    assert D.dropout_loop_chunk([97, 97, 97], {(97, 97): 256}, 0, seed, th)[:2] == ([97, 256], [0, 1])
    # all chunks at once against chunk by chunk
    data, off, merges = D.many_chunk_text()
    for th in (0, D.threshold_of(0.1), 1 << 31):
        want, want_pos, _, passes = D.dropout_loop_chunks(data, off, merges, 5, th)
        tok, _, pos, pass_tokens = D.reference(data, off, merges, 5, th)
        assert np.array_equal(tok, want) and np.array_equal(pos, want_pos) and len(pass_tokens) == passes
    assert np.array_equal(D.reference(data, off, merges, 5, 0)[0], R.rank_loop_text(*R.token_stream(data, off), merges)[0])


# ---- the host loop through the C-ABI -----------------------------------------------------------------------------------

PS = (0.0, 0.1, 0.5, 1.0)


@pytest.fixture(scope="module")
def shakespeare():
    pattern, _, merges = O.parse_model(read_golden("shakespeare_gpt4_lexical_512.model"))
    text = read_data("shakespeare.txt")[:65536]
    off = mbpe.presplit(pattern, np.frombuffer(text, dtype=np.uint8))
    tok = mbpe.Tokenizer(pattern)
    tok.set_merges(merges)
    yield tok, merges, text, text, off, {}
    tok.close()


@pytest.fixture(scope="module")
def special_sample():
    pattern, _, merges = O.parse_model(read_golden("taylorswift_gpt4_first_512.model"))
    text = read_data("specialtokensample.txt")
    specials = parse_special(read_data("special1.txt"))
    buf, off = _special_chunks(pattern, text, specials)        # the chunk buffer: matches and "\0<id>" markers
    tok = mbpe.Tokenizer(pattern)
    tok.set_special_tokens_from_file(read_data("special1.txt"))
    tok.set_merges(merges)
    yield tok, merges, text, buf, off, specials
    tok.close()


@pytest.mark.parametrize("which", ["shakespeare", "special_sample"])
@pytest.mark.parametrize("p", PS)
def test_host_loop_equals_the_oracle(request, which, p):
    tok, merges, text, buf, off, specials = request.getfixturevalue(which)
    seed = 7
    want = D.reference(buf, off, merges, seed, D.threshold_of(p))[0]
    got = tok.encode(text, order="rank", dropout=p, seed=seed)
    assert np.array_equal(got, want)
    assert tok.decode(got) == text
    if p == 0.0:
        assert np.array_equal(got, tok.encode(text, order="rank"))
    else:
        assert not np.array_equal(got, tok.encode(text, order="rank"))
        other = tok.encode(text, order="rank", dropout=p, seed=seed + 1)
        assert np.array_equal(other, D.reference(buf, off, merges, seed + 1, D.threshold_of(p))[0])
        assert (p == 1.0) == np.array_equal(other, got)                    # p = 1 drops whatever the seed
    if p == 1.0:
        # the bytes, and special ids where they occur
        assert np.array_equal(got, D.token_stream(buf, off)[0])
        extra = set(got.tolist()) - set(range(256))
        assert extra <= set(specials.values()) and bool(extra) == bool(specials)
    assert np.array_equal(tok.encode(text, order="rank"), R.rank_loop_text(*R.token_stream(buf, off), merges)[0])


@pytest.mark.parametrize("which", ["shakespeare", "special_sample"])
@pytest.mark.parametrize("p", PS)
def test_host_loop_byte_ranges(request, which, p):
    tok, merges, text, buf, off, specials = request.getfixturevalue(which)
    got, ranges = tok.encode(text, order="rank", dropout=p, seed=7, byte_ranges=True)
    assert np.array_equal(got, tok.encode(text, order="rank", dropout=p, seed=7))
    vocab = vocab_bytes(np.asarray(merges).reshape(-1, 2).tolist())
    names = {v: k for k, v in specials.items()}
    r = ranges.astype(np.int64)
    assert len(r) == len(got) and r[0, 0] == 0 and r[-1, 1] == len(text) and (r[1:, 0] >= r[:-1, 1]).all()
    for j, tk in enumerate(got.tolist()):
        assert text[r[j, 0]:r[j, 1]] == (names[tk] if tk in names else vocab[tk]), j


def test_greedy_order_with_dropout_is_an_error(shakespeare):
    tok, _, text = shakespeare[:3]
    for kw in ({}, {"byte_ranges": True}):
        with pytest.raises(mbpe.MbpeError) as e:
            tok.encode(text[:1000], order="greedy", dropout=0.1, **kw)
        assert e.value.code == mbpe.ERR_ARG and "rank" in str(e.value)
    # p = 0 with the greedy order is today's call, and the tokenizer stays usable
    assert np.array_equal(tok.encode(text[:1000], order="greedy", dropout=0.0), tok.encode(text[:1000]))
    with pytest.raises(mbpe.MbpeError) as e:
        tok.encode(text[:1000], order="rank", dropout=1.5)
    assert e.value.code == mbpe.ERR_ARG
    with pytest.raises(mbpe.MbpeError) as e:
        mbpe._check(mbpe.lib().mbpe_tok_set_encode_dropout(tok._h, (1 << 32) + 1, 0))
    assert e.value.code == mbpe.ERR_ARG
