"""Encoding through the distinct chunks from the Tokenizer and the command line: Tokenizer.encode(device=0, dedup=True)
against the host loop Tokenizer.encode(text), with the host split, the device split and its unicode option, in both
orders and with special tokens; the batch calls against their dedup=False results; what is refused; and --dedup of the
command line, whose output file must be the one it writes without the flag."""
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
SPLITS = (False, True, "unicode")


@pytest.fixture(scope="module")
def tok():
    t = mbpe.Tokenizer(O.GPT4_SPLIT_PATTERN)
    t.set_special_tokens_from_file(read_data("special1.txt"))
    t.set_merges(O.parse_model(read_golden("taylorswift_gpt4_lexical_512.model"))[2])
    yield t
    t.close()


TEXTS = {"taylorswift": lambda: read_data("taylorswift.txt"),
         "specialtokensample": lambda: read_data("specialtokensample.txt"),
         "special1": lambda: read_data("special1.txt")}


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name", sorted(TEXTS))
def test_encode_equals_the_host_loop(tok, name, order):
    text = TEXTS[name]()
    want = tok.encode(text, order=order)                             # the host loop
    assert len(want) > 0
    for split in SPLITS:
        got = tok.encode(text, device=0, device_split=split, order=order, dedup=True)
        assert np.array_equal(got, want), (name, order, split)
        assert np.array_equal(tok.encode(text, device=0, device_split=split, order=order), want)
    assert np.array_equal(tok.encode(text, order=order, dedup=True), want)      # the host loop is unaffected


@pytest.mark.parametrize("order", ORDERS)
def test_batch_calls_equal_their_plain_results(tok, order):
    texts = [read_data("specialtokensample.txt"), b"", read_data("taylorswift.txt")[:20000], b"<|endoftext|>",
             read_data("taylorswift.txt")[5000:9000], read_data("special1.txt")]
    host = [tok.encode(t, order=order) for t in texts]
    for split in SPLITS:
        plain = tok.encode_batch(texts, device_split=split, order=order)
        got = tok.encode_batch(texts, device_split=split, order=order, dedup=True)
        assert [g.tolist() for g in got] == [p.tolist() for p in plain] == [h.tolist() for h in host], split
        for kw in (dict(seq_len=48, layout="packed", pad_id=0, eos_id=100257),
                   dict(seq_len=64, layout="padded", pad_id=0, bos_id=100257)):
            ids, lengths = tok.encode_batch_padded(texts, device_split=split, order=order, **kw)
            ids_d, lengths_d = tok.encode_batch_padded(texts, device_split=split, order=order, dedup=True, **kw)
            assert np.array_equal(ids, ids_d) and np.array_equal(lengths, lengths_d), (split, kw)
            aux = tok.encode_batch_aux(texts, device_split=split, order=order, labels=True, positions=True,
                                       segments=True, **kw)
            aux_d = tok.encode_batch_aux(texts, device_split=split, order=order, labels=True, positions=True,
                                         segments=True, dedup=True, **kw)
            assert sorted(aux) == sorted(aux_d)
            for k in aux:
                assert np.array_equal(aux[k], aux_d[k]), (split, kw, k)
            assert np.array_equal(aux_d["ids"], ids)


def test_what_is_refused(tok):
    text = read_data("taylorswift.txt")[:5000]
    want = tok.encode(text, order="rank")
    for split in (False, True):
        for call in (lambda: tok.encode(text, device=0, device_split=split, order="rank", dedup=True, dropout=0.5, seed=1),
                     lambda: tok.encode(text, device=0, device_split=split, order="rank", dedup=True, byte_ranges=True),
                     lambda: tok.encode_batch([text, text], device_split=split, order="rank", dedup=True, byte_ranges=True),
                     lambda: tok.encode_batch([text, text], device_split=split, order="rank", dedup=True, dropout=0.5),
                     lambda: tok.encode_batch_padded([text], 32, device_split=split, order="rank", dedup=True, dropout=0.5)):
            with pytest.raises(mbpe.MbpeError) as e:
                call()
            assert e.value.code == mbpe.ERR_ARG, split
            assert np.array_equal(tok.encode(text, device=0, device_split=split, order="rank", dedup=True), want)
    # on the host loop both still work while the flag is given
    toks, ranges = tok.encode(text, order="rank", dedup=True, byte_ranges=True)
    assert np.array_equal(toks, want) and ranges[-1, 1] == len(text)
    with pytest.raises(mbpe.MbpeError) as e:
        mbpe._check(mbpe.lib().mbpe_tok_set_encode_dedup(tok._h, 2))
    assert e.value.code == mbpe.ERR_ARG


def test_command_line(tok, tmp_path):
    model = tmp_path / "m.model"
    tok.save(model)
    src = tmp_path / "in.txt"
    src.write_bytes(read_data("specialtokensample.txt") + read_data("taylorswift.txt")[:60000])
    special = tmp_path / "special.txt"
    special.write_bytes(read_data("special1.txt"))

    def run(flags):
        out = tmp_path / "enc"
        if out.exists():
            out.unlink()
        r = subprocess.run([CLI, "--encode", "--input", str(src), "--model-path", str(model), "--output", str(out)] +
                           flags, capture_output=True, text=True)
        return r, (out.read_bytes() if out.exists() else None)

    for order in ([], ["--rank-order"]):
        r, want = run(order)                                         # the host loop
        assert r.returncode == 0 and want
        for dev_flags in (["--device-encode"], ["--device-encode", "--device-split"],
                          ["--device-encode", "--device-split-unicode"]):
            r, plain = run(order + dev_flags)
            assert r.returncode == 0 and plain == want, (order, dev_flags, r.stdout + r.stderr)
            r, got = run(order + dev_flags + ["--dedup"])
            assert r.returncode == 0 and "Success" in r.stdout, r.stdout + r.stderr
            assert got == want, (order, dev_flags)
        r, got = run(order + ["--dedup"])                            # without --device-encode: no effect
        assert r.returncode == 0 and got == want
    # with --dropout or --byte-ranges-out: the library's error and a non-zero exit
    r, got = run(["--rank-order", "--device-encode", "--dedup", "--dropout", "0.5"])
    assert r.returncode != 0 and "dedup" in r.stderr and got is None
    r, got = run(["--device-encode", "--dedup", "--byte-ranges-out", str(tmp_path / "ranges")])
    assert r.returncode != 0 and "dedup" in r.stderr and got is None
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert "--dedup" in r.stdout and "--device-encode" in r.stdout.split("--dedup", 1)[1]
