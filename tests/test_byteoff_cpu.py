"""Token byte ranges on the host (mbpe_tok_encode_byteoff with device_id -1; Tokenizer.encode(byte_ranges=True)):
against the position-carrying BPE of byteoff_cases.py, as properties that need no reference, on the inputs where the
original text and the encoder's text differ (special tokens, gapped patterns, NUL-led parts), and the argument
errors.  Plus the 64-bit scan arithmetic of csrc/span.h built by a host compiler.  No GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import mbpe
from byteoff_cases import parse_model, parse_special, tokenizer_encode, vocab_bytes
from conftest import read_data, read_golden

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "minbpe-cc_amd", "csrc")
ORDERS = ("greedy", "rank")


def _tokenizer(model, special_raw=None, pattern=None):
    pat, merges = parse_model(read_golden(model + ".model"))
    tok = mbpe.Tokenizer(pat if pattern is None else pattern)
    tok.set_merges(np.array(merges, dtype=np.uint32))
    special = {}
    if special_raw is not None:
        tok.set_special_tokens_from_file(special_raw)
        special = parse_special(special_raw)
    return tok, (pat if pattern is None else pattern), special, merges


def _taylor_slice():
    return read_data("taylorswift.txt")[:16384].decode("utf-8", "ignore").encode("utf-8")


def _cases():
    sp = read_data("special1.txt")
    yield "sample/basic", "shakespeare_basic_lexical_512", None, read_data("sample.txt")[:4096]
    yield "special/gpt4", "taylorswift_gpt4_first_512", sp, read_data("specialtokensample.txt")
    yield "special1-as-text/gpt4", "taylorswift_gpt4_first_512", sp, sp
    yield "taylor/gpt4", "taylorswift_gpt4_lexical_512", None, _taylor_slice()


CASES = list(_cases())


def check_properties(text, tokens, ranges, merges, special, tiles):
    """ranges ascend without overlap; text[s:e] is the id's vocabulary entry or the special's name."""
    vocab = vocab_bytes(merges)
    names = {v: k for k, v in special.items()}
    r = ranges.astype(np.int64)
    assert r.shape == (len(tokens), 2)
    assert (r[:, 0] <= r[:, 1]).all()
    assert (r[1:, 0] >= r[:-1, 1]).all()
    assert len(r) == 0 or (r[0, 0] >= 0 and r[-1, 1] <= len(text))
    for t, (s, e) in zip(tokens.tolist(), r.tolist()):
        assert text[s:e] == (names[t] if t in names else vocab[t]), (t, s, e)
    if tiles:
        assert len(r) == 0 or (r[0, 0] == 0 and r[-1, 1] == len(text))
        assert (r[1:, 0] == r[:-1, 1]).all()


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_host_loop_equals_the_position_carrying_reference(case, order):
    _, model, sp, text = case
    tok, pat, special, merges = _tokenizer(model, sp)
    tokens, ranges = tok.encode(text, order=order, byte_ranges=True)
    want_t, want_r = tokenizer_encode(text, pat, special, merges, rank=order == "rank")
    assert tokens.tolist() == want_t.tolist()
    assert ranges.tolist() == want_r.tolist()
    assert tokens.tolist() == tok.encode(text, order=order).tolist()          # the plain call's tokens
    check_properties(text, tokens, ranges, merges, special, tiles=sp is None)


def test_greedy_on_the_whole_sample_as_one_chunk():
    text = read_data("sample.txt")
    tok, pat, special, merges = _tokenizer("shakespeare_basic_lexical_512")
    tokens, ranges = tok.encode(text, byte_ranges=True)
    want_t, want_r = tokenizer_encode(text, pat, special, merges)
    assert len(tokens) == 15677
    assert tokens.tolist() == want_t.tolist() and ranges.tolist() == want_r.tolist()
    check_properties(text, tokens, ranges, merges, special, tiles=True)


def test_gapped_pattern_leaves_the_gap_bytes_to_no_token():
    text = b"abc123def 45 gh7"
    tok, pat, special, merges = _tokenizer("taylorswift_basic_lexical_512", pattern="[a-z]+")
    tokens, ranges = tok.encode(text, byte_ranges=True)
    want_t, want_r = tokenizer_encode(text, pat, special, merges)
    assert tokens.tolist() == want_t.tolist() and ranges.tolist() == want_r.tolist()
    check_properties(text, tokens, ranges, merges, special, tiles=False)
    covered = np.zeros(len(text), dtype=bool)
    for s, e in ranges.tolist():
        covered[s:e] = True
    assert covered.tolist() == [chr(c).islower() for c in text]


E, F = b"<|endoftext|>", b"<|fim_prefix|>"


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("text", [E + b" starts here", b"it ends with " + E, b"two " + E + F + b" in a row", E + F, E, b"",
                                  b"x", b"the tail of one: <|endoftext", b"\x0042", b"\x00 +17 and more",
                                  b"\x00no number", b"a " + E + b"\x007" + F],
                         ids=["first", "last", "adjacent", "only-two", "only-one", "empty", "one-byte", "partial-name",
                              "nul-number", "nul-blank-number", "nul-no-number", "nul-between-specials"])
def test_special_tokens_and_nul_led_parts(text, order):
    tok, pat, special, merges = _tokenizer("taylorswift_gpt4_first_512", read_data("special1.txt"))
    tokens, ranges = tok.encode(text, order=order, byte_ranges=True)
    want_t, want_r = tokenizer_encode(text, pat, special, merges, rank=order == "rank")
    assert tokens.tolist() == want_t.tolist()
    assert ranges.tolist() == want_r.tolist()
    assert tokens.tolist() == tok.encode(text, order=order).tolist()
    for t, (s, e) in zip(tokens.tolist(), ranges.tolist()):
        if t in special.values():
            assert special[text[s:e]] == t                         # a special's range is its name's occurrence


def test_a_nul_led_part_is_one_token_over_its_whole_part():
    # no pattern: the part "\0 42abc" is one chunk, std::stoi takes 42, and token 42 ('*') covers all seven bytes
    tok, pat, special, merges = _tokenizer("taylorswift_basic_lexical_512")
    tokens, ranges = tok.encode(b"\x00 42abc", byte_ranges=True)
    assert tokens.tolist() == [42] and ranges.tolist() == [[0, 7]]


def test_argument_errors():
    L = mbpe.lib()
    tok, _, _, _ = _tokenizer("taylorswift_gpt4_lexical_512")
    text = np.frombuffer(b"hello world, hello", dtype=np.uint8)
    want = tok.encode(text)
    n = ctypes.c_uint64(99)
    out = np.full(64, 0xABABABAB, dtype=np.uint32)
    ranges = np.full(128, 0xCDCDCDCD, dtype=np.uint64)
    args = (tok._h, text.ctypes.data, len(text), 0, -1)
    # the query
    assert L.mbpe_tok_encode_byteoff(*args, None, None, 0, ctypes.byref(n)) == mbpe.OK
    assert n.value == len(want)
    # a cap too small: the count, and neither a token nor a range
    assert L.mbpe_tok_encode_byteoff(*args, out.ctypes.data, ranges.ctypes.data, len(want) - 1,
                                     ctypes.byref(n)) == mbpe.ERR_ARG
    assert n.value == len(want)
    assert (out == 0xABABABAB).all() and (ranges == 0xCDCDCDCD).all()
    # NULL outputs
    assert L.mbpe_tok_encode_byteoff(*args, out.ctypes.data, None, 64, ctypes.byref(n)) == mbpe.ERR_ARG
    assert L.mbpe_tok_encode_byteoff(*args, out.ctypes.data, ranges.ctypes.data, 64, None) == mbpe.ERR_ARG
    assert L.mbpe_tok_encode_byteoff(None, text.ctypes.data, len(text), 0, -1, out.ctypes.data, ranges.ctypes.data, 64,
                                     ctypes.byref(n)) == mbpe.ERR_ARG
    assert L.mbpe_tok_encode_byteoff(tok._h, None, 5, 0, -1, out.ctypes.data, ranges.ctypes.data, 64,
                                     ctypes.byref(n)) == mbpe.ERR_ARG
    assert (out == 0xABABABAB).all() and (ranges == 0xCDCDCDCD).all()
    # the batch call has no host loop
    doc_off = np.array([0, len(text)], dtype=np.uint64)
    assert L.mbpe_tok_encode_batch_byteoff_device(tok._h, text.ctypes.data, doc_off.ctypes.data, 1, 0, -1, out.ctypes.data,
                                                  ranges.ctypes.data, 64, None, ctypes.byref(n)) == mbpe.ERR_ARG
    # and the exact fit
    assert L.mbpe_tok_encode_byteoff(*args, out.ctypes.data, ranges.ctypes.data, len(want), ctypes.byref(n)) == mbpe.OK
    assert out[:n.value].tolist() == want.tolist()


FLAGS = {
    "plain": ["-O2"],
    "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
}


@pytest.mark.parametrize("build", sorted(FLAGS))
def test_scan_arithmetic_in_64_bits(build, tmp_path):
    exe = str(tmp_path / "byteoff_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Wextra", "-Werror"] + FLAGS[build] +
                          ["-I" + CSRC, os.path.join(HERE, "byteoff_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    # 10 span counts x 4 kinds of counts + 6 index lists x 2,000 queries
    assert r.stdout.strip().endswith("ok: %d cases, 0 failures" % (10 * 4 + 6 * 2000))
