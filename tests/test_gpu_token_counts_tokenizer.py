"""Tokenizer.token_counts and the command line's --token-counts-out on the device: one and the same table on every route
-- the host loop, the device over the host split, the device split (ASCII and unicode), each with and without "dedup", in
both orders -- and that table is the bincount of Tokenizer.encode_batch.  The texts are the first 64 KiB of the golden
shakespeare and taylorswift texts, cut into documents with <|endoftext|> between and inside them, under the golden gpt4
models with that special token registered (id 100,257, far above 256 + n_merges)."""
import os
import subprocess

import numpy as np
import pytest

import mbpe
import oracle as O
from conftest import ROOT, read_data, read_golden

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CLI = os.path.join(ROOT, "minbpe-cc_amd", "minbpe-cc")
ORDERS = ("greedy", "rank")
CORPORA = ("shakespeare", "taylorswift")
EOT = b"<|endoftext|>"
N_IDS = 100258


def tokenizer(corpus):
    tok = mbpe.Tokenizer(O.GPT4_SPLIT_PATTERN)
    tok.set_special_tokens_from_file(EOT + b" 100257\n")
    tok.set_merges(O.parse_model(read_golden(corpus + "_gpt4_lexical_512.model"))[2])
    return tok


def documents(corpus):
    data = read_data(corpus + ".txt")[:65536]
    return [data[:30000], EOT + data[30000:50000], b"", data[50000:60000] + EOT + EOT + data[60000:], EOT]


@pytest.fixture(scope="module", params=[(c, o) for c in CORPORA for o in ORDERS], ids=lambda p: "%s-%s" % p)
def case(request):
    """(tokenizer, texts, order, the table of encode_batch), computed once per corpus and order."""
    torch.cuda.set_device(0)
    corpus, order = request.param
    tok, texts = tokenizer(corpus), documents(corpus)
    want = np.zeros(N_IDS, dtype=np.uint64)
    for ids in tok.encode_batch(texts, order=order):
        want += np.bincount(ids, minlength=N_IDS).astype(np.uint64)
    assert want[100257] == 4 and want[:256].sum() > 0 and want[256:512].sum() > 0
    want.setflags(write=False)
    return tok, texts, order, want


def test_host_loop(case):
    tok, texts, order, want = case
    assert np.array_equal(tok.token_counts(texts, device=None, order=order), want)


@pytest.mark.parametrize("dedup", [False, True])
@pytest.mark.parametrize("split", [False, True, "unicode"])
def test_device_routes(case, split, dedup):
    tok, texts, order, want = case
    got = tok.token_counts(texts, device=0, device_split=split, order=order, dedup=dedup)
    assert got.dtype == np.uint64 and np.array_equal(got, want)


@pytest.mark.parametrize("split", [False, True])
def test_batches_and_repeats(case, split):
    tok, texts, order, want = case
    got = tok.token_counts(iter(texts), device=0, device_split=split, order=order, dedup=True, batch_bytes=25000)
    assert np.array_equal(got, want)
    reps = [2, 1, 5, 1, 3]
    both = np.zeros(N_IDS, dtype=np.uint64)
    for ids, r in zip(tok.encode_batch(texts, order=order), reps):
        both += np.bincount(ids, minlength=N_IDS).astype(np.uint64) * np.uint64(r)
    assert np.array_equal(tok.token_counts(texts, device=0, device_split=split, order=order, repeats=reps), both)
    with pytest.raises(mbpe.MbpeError) as e:
        tok.token_counts(texts, device=0, device_split=split, order=order, repeats=[1, 1, 0, 1, 1])
    assert e.value.code == mbpe.ERR_ARG


@pytest.mark.parametrize("order", ORDERS)
def test_cli_writes_the_same_file_on_every_route(order, tmp_path):
    torch.cuda.set_device(0)
    tok = tokenizer("taylorswift")
    model = str(tmp_path / "sp.model")
    tok.save(model)
    text = b"".join(documents("taylorswift"))
    sample = str(tmp_path / "in.txt")
    open(sample, "wb").write(text)
    want = np.bincount(tok.encode(text, order=order), minlength=N_IDS)
    flags = ["--rank-order"] if order == "rank" else []
    files = {}
    for name, route in (("host", []), ("device", ["--device-encode"]), ("split", ["--device-encode", "--device-split"]),
                        ("dedup", ["--device-encode", "--dedup"]),
                        ("split-dedup", ["--device-encode", "--device-split-unicode", "--dedup"])):
        out = str(tmp_path / (name + ".counts"))
        r = subprocess.run([CLI, "--encode", "--input", sample, "--model-path", model, "--token-counts-out", out] + flags + route,
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        files[name] = open(out, "rb").read()
    rows = files["host"].decode().splitlines()
    assert len(rows) == N_IDS and rows[0].startswith("0 ") and rows[-1] == "100257 4"
    assert [int(r.split()[1]) for r in rows] == want.tolist()
    for name in files:
        assert files[name] == files["host"], name
