"""Word counts across pieces, without a GPU: the host restatement of csrc/wordcount.h as a stand-alone program (plain and
under ASan + UBSan) against a std::map; the Python accumulator of tests/wordcount_cases.py against one dedup of the
concatenated list; the C-ABI's argument checks, which come before the device is touched; and the cut of the golden
texts that the tokenizer tests rely on."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import mbpe
import oracle as O
import dedup_cases as C
import wordcount_cases as W
from conftest import read_data

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "minbpe-cc_amd", "csrc")

FLAGS = {
    "plain": ["-O2"],
    "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
}


@pytest.mark.parametrize("build", sorted(FLAGS))
def test_wordcount_host_restatement(build, tmp_path):
    exe = str(tmp_path / "wordcount_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Wextra", "-Werror"] + FLAGS[build] +
                          ["-I" + CSRC, os.path.join(HERE, "wordcount_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.strip().endswith("0 failures")


def _same(pieces, max_chunk_bytes=C.MAX_CHUNK_BYTES):
    got = W.accumulate(pieces, max_chunk_bytes)
    assert got == C.dedup(W.concat(pieces), max_chunk_bytes)
    return got


def test_python_accumulator_small():
    u, w, f = _same([[b"ab", b"c", b"ab"], [], [b"ab", b"d", b"c"]])
    assert u == [b"ab", b"c", b"d"] and w == [3, 2, 1] and f == [0, 1, 4]
    long = b"x" * 5
    u, w, f = _same([[long, b"a"], [long, b"a"]], max_chunk_bytes=4)
    assert u == [long, b"a", long] and w == [1, 2, 1] and f == [0, 1, 2]
    assert W.accumulate([]) == ([], [], []) and W.accumulate([[], []]) == ([], [], [])
    acc = W.Accumulator()
    acc.add([b"a", b"b", b"a"], repeat=3)
    acc.add([b"b"])
    assert acc.result() == ([b"a", b"b"], [6, 4], [0, 1]) and acc.n_chunks_total == 10 and acc.n_pieces == 2


@pytest.mark.parametrize("n_pieces", [1, 2, 7])
@pytest.mark.parametrize("seed", range(6))
def test_python_accumulator_equals_one_dedup(seed, n_pieces):
    rng = np.random.default_rng(40 + seed)
    chunks = C.random_chunks(seed, int(rng.integers(50, 1500)), 12, int(rng.integers(1, 5)))
    pieces = W.cut_list(chunks, n_pieces)
    pieces.insert(len(pieces) // 2, [])
    _same(pieces)


def test_python_accumulator_other_generators():
    for d in (-1, 0, 1):
        chunks = C.edge_chunks(3, 16 * 40 + d)
        _same([chunks[0::3], chunks[1::3] + chunks[2::3]])
    long = C.long_chunks()
    u, w, _ = _same([long[:5], long[5:]])
    assert [len(c) for c in u].count(C.MAX_CHUNK_BYTES + 1) == 2 and sum(w) == len(long)
    _same([C.distinct_chunks(2336)[a:b] for a, b in ((0, 16), (16, 80), (80, 336), (336, 2336), (0, 16))])


def _code(rc, want, word=None):
    assert rc == want, (rc, mbpe.lib().mbpe_last_error())
    if word:
        assert word in mbpe.lib().mbpe_last_error().decode()


def test_c_abi_checks_arguments_before_the_device():
    L = mbpe.lib()
    n = ctypes.c_uint64()
    off = np.zeros(2, dtype=np.uint64)
    _code(L.mbpe_wordcount_create(0, None), mbpe.ERR_ARG)
    _code(L.mbpe_wordcount_add(None, None, 0, 0, off.ctypes.data, 1, 1, ctypes.byref(n), None), mbpe.ERR_ARG, "NULL")
    _code(L.mbpe_wordcount_add(None, None, 0, 0, off.ctypes.data, 1, 0, ctypes.byref(n), None), mbpe.ERR_ARG, "repeat")
    _code(L.mbpe_wordcount_add_endmask(None, None, 0, None, 1, ctypes.byref(n), None), mbpe.ERR_ARG, "NULL")
    _code(L.mbpe_wordcount_add_endmask(None, None, 0, None, 0, ctypes.byref(n), None), mbpe.ERR_ARG, "repeat")
    _code(L.mbpe_wordcount_result(None, None, None, None, None), mbpe.ERR_ARG)
    _code(L.mbpe_wordcount_get(None, None, None, None, None, 0, 0), mbpe.ERR_ARG)
    _code(L.mbpe_wordcount_stats(None, None, None, None, None), mbpe.ERR_ARG)
    _code(L.mbpe_wordcount_reset(None), mbpe.ERR_ARG)
    _code(L.mbpe_wordcount_kernel_ms(None, None), mbpe.ERR_ARG)
    _code(L.mbpe_wordcount_alloc_count(None, None), mbpe.ERR_ARG)
    for name, value in ((b"hash_bits", 65), (b"hash_bits", -1), (b"max_chunk_bytes", -1), (b"max_chunk_bytes", 1 << 31),
                        (b"map", 1), (b"no_such_option", 1)):
        _code(L.mbpe_wordcount_set_option(None, name, value), mbpe.ERR_ARG, "bad value")
    _code(L.mbpe_wordcount_set_option(None, None, 1), mbpe.ERR_ARG, "NULL")
    _code(L.mbpe_wordcount_set_option(None, b"hash_bits", 4), mbpe.ERR_ARG, "NULL")
    L.mbpe_wordcount_destroy(None)


def test_tokenizer_pieces_need_a_session():
    L = mbpe.lib()
    tok = mbpe.Tokenizer(O.GPT4_SPLIT_PATTERN)
    text = np.frombuffer(b"hello world", dtype=np.uint8)
    _code(L.mbpe_tok_train_pieces_add(tok._h, text.ctypes.data, len(text), 1), mbpe.ERR_STATE, "session")
    _code(L.mbpe_tok_train_pieces_finish(tok._h, 300, 1, 0, 0), mbpe.ERR_STATE, "session")
    _code(L.mbpe_tok_train_pieces_abort(tok._h), mbpe.OK)
    _code(L.mbpe_tok_train_pieces_add(None, text.ctypes.data, len(text), 1), mbpe.ERR_ARG)
    _code(L.mbpe_tok_train_pieces_add(tok._h, None, 3, 1), mbpe.ERR_ARG)
    _code(L.mbpe_tok_train_pieces_begin(None, 0, 0), mbpe.ERR_ARG)
    assert len(tok.merges()) == 0
    tok.close()


@pytest.mark.parametrize("encoder", ["gpt2", "gpt4"])
@pytest.mark.parametrize("text", ["taylorswift.txt", "shakespeare.txt"])
def test_cut_keeps_the_chunk_list(text, encoder):
    """The precondition of the tokenizer tests: cut where a letter or digit is followed by whitespace, the pieces' chunk
    lists laid end to end are the whole text's."""
    data = read_data(text)
    pattern = O.GPT4_SPLIT_PATTERN if encoder == "gpt4" else O.GPT2_SPLIT_PATTERN
    pieces = W.cut_text(data, 5)
    assert b"".join(pieces) == data and all(len(p) > len(data) // 10 for p in pieces)
    whole = C.chunks_of(data, mbpe.presplit(pattern, data))
    parts = [C.chunks_of(p, mbpe.presplit(pattern, p)) for p in pieces]
    assert W.concat(parts) == whole
    assert W.accumulate(parts) == C.dedup(whole)
