"""Token byte ranges at the Tokenizer level on the GPU: the host loop, the device with the host split, the device
with the device split and its "unicode" form agree token for token and range for range; the batch call equals the
single-text call; a gapped pattern; the command line's --byte-ranges-out."""
import os
import subprocess

import numpy as np
import pytest

import mbpe
from byteoff_cases import parse_model, vocab_bytes
from conftest import DATA, ROOT, read_data, read_golden

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "minbpe-cc_amd", "minbpe-cc")
SPECIAL = {b"<|endoftext|>": 100257, b"<|fim_prefix|>": 100258, b"<|fim_middle|>": 100259, b"<|fim_suffix|>": 100260,
           b"<|endofprompt|>": 100276}


@pytest.fixture(scope="module")
def dev():
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def tokenizer(model):
    pat, merges = parse_model(read_golden(model + ".model"))
    t = mbpe.Tokenizer(pat)
    t.set_special_tokens_from_file(read_data("special1.txt"))
    t.set_merges(np.array(merges, dtype=np.uint32))
    return t, merges


CASES = [("specialtokensample.txt", "taylorswift_gpt4_first_512"), ("taylorswift.txt", "taylorswift_gpt4_lexical_512"),
         ("shakespeare.txt", "taylorswift_gpt2_lexical_512")]


@pytest.fixture(scope="module", params=CASES, ids=[c[0] for c in CASES])
def case(request, dev):
    name, model = request.param
    t, merges = tokenizer(model)
    return t, merges, read_data(name)


@pytest.mark.parametrize("order", ["greedy", "rank"])
def test_the_routes_agree(case, order):
    t, merges, text = case
    want_t, want_r = t.encode(text, order=order, byte_ranges=True)              # the host loop
    assert want_t.tolist() == t.encode(text, order=order).tolist()
    # what the host loop gives, as properties: the ranges ascend, and text[s:e] is the token's entry or its name
    r = want_r.astype(np.int64)
    assert (r[1:, 0] >= r[:-1, 1]).all() and r[0, 0] == 0 and r[-1, 1] == len(text)
    vocab = vocab_bytes(merges)
    names = {v: k for k, v in SPECIAL.items()}
    at = np.random.default_rng(3).integers(0, len(r), 2000)
    for j in at.tolist():
        tk = int(want_t[j])
        assert text[r[j, 0]:r[j, 1]] == (names[tk] if tk in names else vocab[tk])
    for split in (False, True, "unicode"):
        got_t, got_r = t.encode(text, device=0, device_split=split, order=order, byte_ranges=True)
        assert np.array_equal(got_t, want_t), split
        assert got_r.shape == want_r.shape and np.array_equal(got_r, want_r), split


NUL_TEXT = b"hi<|endoftext|>\x0042 x<|fim_prefix|>\x00abc  <|endoftext|><|endoftext|>  \x00 7<|endofprompt|>tail  "


@pytest.mark.parametrize("split", [False, True, "unicode"], ids=["host-split", "device-split", "unicode"])
def test_batch_equals_the_single_text_call(dev, split):
    t, _ = tokenizer("taylorswift_gpt4_lexical_512")
    swift = read_data("taylorswift.txt")
    texts = [read_data("specialtokensample.txt"), b"", swift[:5000], b"<|endoftext|>", NUL_TEXT,
             swift[5000:9000] + b"<|endoftext|>", b"a  ", b""]
    got = t.encode_batch(texts, device_split=split, byte_ranges=True)
    plain = t.encode_batch(texts, device_split=split)
    assert len(got) == len(texts)
    for text, (tokens, ranges), p in zip(texts, got, plain):
        want_t, want_r = t.encode(text, byte_ranges=True)                        # the host loop on that text alone
        assert tokens.tolist() == want_t.tolist() == p.tolist()
        assert ranges.shape == want_r.shape and ranges.tolist() == want_r.tolist()
        one_t, one_r = t.encode(text, device=0, device_split=split, byte_ranges=True)
        assert one_t.tolist() == want_t.tolist() and one_r.tolist() == want_r.tolist()
    assert got[3][0].tolist() == [100257] and got[3][1].tolist() == [[0, 13]]
    assert got[1][0].tolist() == [] and got[1][1].shape == (0, 2)


def test_a_gapped_pattern(dev):
    _, merges = parse_model(read_golden("taylorswift_basic_lexical_512.model"))
    t = mbpe.Tokenizer("[a-z]+")
    t.set_merges(np.array(merges, dtype=np.uint32))
    text = b"the 12 quick brown 3456 foxes7and8the lazy dogs 9"
    want_t, want_r = t.encode(text, byte_ranges=True)
    got_t, got_r = t.encode(text, device=0, byte_ranges=True)
    assert got_t.tolist() == want_t.tolist() and got_r.tolist() == want_r.tolist()
    covered = np.zeros(len(text), dtype=bool)
    for s, e in got_r.tolist():
        covered[s:e] = True
    assert covered.tolist() == [chr(c).islower() for c in text]
    with pytest.raises(mbpe.MbpeError) as e:                                     # no device split for a custom pattern
        t.encode(text, device=0, device_split=True, byte_ranges=True)
    assert e.value.code == mbpe.ERR_ARG


@pytest.mark.parametrize("rank", [False, True], ids=["greedy", "rank"])
def test_cli_byte_ranges_out(dev, tmp_path, rank):
    t, _ = tokenizer("taylorswift_gpt4_first_512")
    model = tmp_path / "m.model"
    t.save(model)
    src = os.path.join(DATA, "specialtokensample.txt")
    want_t, want_r = t.encode(read_data("specialtokensample.txt"), order="rank" if rank else "greedy", byte_ranges=True)
    files = []
    for k, flags in enumerate(([], ["--device-encode"], ["--device-encode", "--device-split"])):
        out, rng = tmp_path / ("enc%d" % k), tmp_path / ("ranges%d" % k)
        r = subprocess.run([CLI, "--encode", "--input", src, "--model-path", str(model), "--output", str(out),
                            "--byte-ranges-out", str(rng)] + flags + (["--rank-order"] if rank else []),
                           capture_output=True, text=True)
        assert r.returncode == 0 and "Success" in r.stdout, r.stdout + r.stderr
        files.append((out.read_bytes(), rng.read_text()))
    assert files[0] == files[1] == files[2]
    tokens = np.frombuffer(files[0][0], dtype="<u4")
    lines = files[0][1].splitlines()
    assert tokens.tolist() == want_t.tolist() and len(lines) == len(tokens)
    assert [[int(v) for v in ln.split()] for ln in lines] == want_r.tolist()
