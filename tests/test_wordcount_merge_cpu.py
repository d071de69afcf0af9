"""Merging word-count tables, without a GPU: the Python rule of tests/wordcount_merge_cases.py against one dedup of the
concatenated list, chain against tree; WordcountHost::merge / to_blob / from_blob of csrc/wordcount.h as a stand-alone
program (plain and under ASan + UBSan) against a std::map, every rule of the blob check included; the Python blob writer
against the layout the header states; and the new C calls' argument checks, which come before the device is touched."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import mbpe
import oracle as O
import dedup_cases as C
import wordcount_cases as W
import wordcount_merge_cases as M

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "minbpe-cc_amd", "csrc")

FLAGS = {
    "plain": ["-O2"],
    "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
}


@pytest.mark.parametrize("build", sorted(FLAGS))
def test_wordcount_merge_host_restatement(build, tmp_path):
    exe = str(tmp_path / "wordcount_merge_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Wextra", "-Werror"] + FLAGS[build] +
                          ["-I" + CSRC, os.path.join(HERE, "wordcount_merge_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.strip().endswith("0 failures")


def _pieces(seed, n_pieces=14):
    rng = np.random.default_rng(70 + seed)
    chunks = C.random_chunks(seed, int(rng.integers(200, 2000)), 12, int(rng.integers(1, 5)))
    pieces = W.cut_list(chunks, n_pieces)
    pieces.insert(n_pieces // 2, [])
    return pieces


def _chain(tables):
    acc = M.count([], tables[0].max_chunk_bytes)
    for t in tables:
        acc.merge(t)
    return acc


def _tree(tables):
    """T0 + (T1 + (T2 + ...)): built from the right, every table freshly copied through an empty one."""
    right = _chain(tables[-1:])
    for t in reversed(tables[:-1]):
        left = _chain([t])
        left.merge(right)
        right = left
    return right


def test_python_merge_small():
    a, b = M.count([[b"ab", b"c", b"ab"]]), M.count([[], [b"d", b"ab", b"c"]])
    a.merge(b)
    assert M.table(a) == ([b"ab", b"c", b"d"], [3, 2, 1], [0, 1, 3], 6, 3)
    long = b"x" * 5
    a, b = M.count([[long, b"a"]], 4), M.count([[long, b"a"]], 4)
    a.merge(b)
    assert M.table(a) == ([long, b"a", long], [1, 2, 1], [0, 1, 2], 4, 2)
    # out of order: the same weights, the first occurrences of that order
    a, b = M.count([[b"p", b"q"]]), M.count([[b"q", b"r"]])
    b.merge(a)
    assert M.table(b) == ([b"q", b"r", b"p"], [2, 1, 1], [0, 1, 2], 4, 2)


@pytest.mark.parametrize("n_tables", [2, 3, 7])
@pytest.mark.parametrize("seed", range(5))
def test_python_merge_equals_one_dedup(seed, n_tables):
    pieces = _pieces(seed)
    tables = [M.count(g) for g in M.groups(pieces, n_tables)]
    whole = M.count(pieces)
    assert whole.result() == C.dedup(W.concat(pieces))
    chain, tree = _chain(tables), _tree(tables)
    assert M.table(chain) == M.table(whole) == M.table(tree)
    assert chain.result() == C.dedup(W.concat(pieces))


def test_python_merge_other_generators():
    for d in (-1, 0, 1):
        chunks = C.edge_chunks(3, 16 * 40 + d)
        pieces = [chunks[0::3], chunks[1::3] + chunks[2::3]]
        assert _chain([M.count([p]) for p in pieces]).result() == C.dedup(W.concat(pieces))
    long = C.long_chunks()
    got = _chain([M.count([long[:5]]), M.count([long[5:]])])
    assert got.result() == C.dedup(long)
    assert [len(c) for c in got.uniq].count(C.MAX_CHUNK_BYTES + 1) == 2
    low = _chain([M.count([long[:5]], C.MAX_CHUNK_BYTES - 1), M.count([long[5:]], C.MAX_CHUNK_BYTES - 1)])
    assert low.result() == C.dedup(long, C.MAX_CHUNK_BYTES - 1)
    chunks = C.distinct_chunks(2336)
    got = _chain([M.count([chunks[:16]]), M.count([chunks[16:]]), M.count([chunks[:16]])])
    assert got.result() == C.dedup(chunks + chunks[:16])
    # repeats on the pieces
    pieces = W.cut_list(C.random_chunks(5, 900, 10, 3), 4)
    reps = [1, 3, 2, 5]
    assert M.table(_chain([M.count(pieces[:2], repeats=reps[:2]), M.count(pieces[2:], repeats=reps[2:])])) == \
        M.table(M.count(pieces, repeats=reps))


def test_python_blob_layout():
    acc = M.count([[b"ab", b"c", b"ab"], [b"c", b"dd"]])
    blob = M.blob_of(acc)
    assert len(blob) == 64 + 3 * 24 + 16
    assert struct.unpack_from("<II7Q", blob) == (M.MAGIC, 1, 256, 3, 5, 2, 5, 5, 0)
    assert blob[:4] == b"MBWC"
    assert struct.unpack_from("<9Q", blob, 64) == (2, 3, 5, 2, 2, 1, 0, 1, 4)
    assert blob[64 + 72:] == b"abcdd" + b"\0" * 11
    bad = M.corrupt_blobs(M.count([C.distinct_chunks(20)]))
    assert len(bad) == 8 and all(b != M.blob_of(M.count([C.distinct_chunks(20)])) for b in bad.values())


def _code(rc, want, word=None):
    assert rc == want, (rc, mbpe.lib().mbpe_last_error())
    if word:
        assert word in mbpe.lib().mbpe_last_error().decode()


def test_c_abi_checks_arguments_before_the_device():
    L = mbpe.lib()
    n = ctypes.c_uint64()
    buf = np.zeros(64, dtype=np.uint8)
    _code(L.mbpe_wordcount_export_size(None, ctypes.byref(n)), mbpe.ERR_ARG, "NULL")
    _code(L.mbpe_wordcount_export(None, buf.ctypes.data, 64, ctypes.byref(n)), mbpe.ERR_ARG, "NULL")
    _code(L.mbpe_wordcount_merge_blob(None, buf.ctypes.data, 64, None, None), mbpe.ERR_ARG, "NULL")
    _code(L.mbpe_wordcount_merge(None, None), mbpe.ERR_ARG, "NULL")
    _code(L.mbpe_tok_train_pieces_export_size(None, ctypes.byref(n)), mbpe.ERR_ARG, "NULL")
    _code(L.mbpe_tok_train_pieces_export(None, buf.ctypes.data, 64, None), mbpe.ERR_ARG, "NULL")
    _code(L.mbpe_tok_train_pieces_merge(None, buf.ctypes.data, 64), mbpe.ERR_ARG, "NULL")


def test_tokenizer_counts_need_a_session():
    L = mbpe.lib()
    tok = mbpe.Tokenizer(O.GPT4_SPLIT_PATTERN)
    n = ctypes.c_uint64()
    buf = np.zeros(64, dtype=np.uint8)
    _code(L.mbpe_tok_train_pieces_export_size(tok._h, ctypes.byref(n)), mbpe.ERR_STATE, "session")
    _code(L.mbpe_tok_train_pieces_export(tok._h, buf.ctypes.data, 64, ctypes.byref(n)), mbpe.ERR_STATE, "session")
    _code(L.mbpe_tok_train_pieces_merge(tok._h, buf.ctypes.data, 64), mbpe.ERR_STATE, "session")
    _code(L.mbpe_tok_train_pieces_merge(tok._h, None, 0), mbpe.ERR_ARG, "NULL")
    assert len(tok.merges()) == 0
    tok.close()
