"""The gpt2 / gpt4 pre-split on the device (mbpe_splitter_*, csrc/split.hip) against mbpe_presplit on the same bytes,
for both patterns: fixtures, fuzz, every length around the block and tile edges, spans the device hands to the host,
whitespace and newlines across block edges, the outputs and their error rules, the trainer's end-mask entry, and the
tokenizer and command line end to end against the golden models."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import mbpe
import oracle as O
import split_cases as S
from conftest import GOLDEN, ROOT, read_data, read_golden

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

ENCODERS = ["gpt2", "gpt4"]
BLOCK, TILE = mbpe.SPLIT_BLOCK, mbpe.SPLIT_TILE
CLI = os.path.join(ROOT, "minbpe-cc_amd", "minbpe-cc")


@pytest.fixture(scope="module")
def dev():
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def splitters(dev):
    sp = {e: mbpe.Splitter(S.PATTERNS[e]) for e in ENCODERS}
    yield sp
    for s in sp.values():
        s.close()


def check(sp, encoder, data):
    """One split with offsets; the truth is mbpe_presplit.  (cap = n_bytes always suffices: no chunk is empty.)"""
    data = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else data
    got = sp.split(data, cap_chunks=len(data))
    want = mbpe.presplit(S.PATTERNS[encoder], data)
    if len(got) != len(want) or (got != want).any():
        k = next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), min(len(got), len(want)))
        raise AssertionError("%s, %d bytes: %d chunks for %d, first difference at chunk %d: %s for %s" % (
            encoder, len(data), len(got) - 1, len(want) - 1, k, got[k:k + 3], want[k:k + 3]))
    return got


@pytest.mark.parametrize("encoder", ENCODERS)
@pytest.mark.parametrize("name,n_host,host_bytes", [("shakespeare.txt", 0, 0), ("taylorswift.txt", 109, 2142),
                                                    ("sample.txt", None, None)])
def test_fixtures(splitters, encoder, name, n_host, host_bytes):
    sp = splitters[encoder]
    sp.set_option("max_span", mbpe.SPLIT_MAX_SPAN)
    check(sp, encoder, read_data(name))
    if n_host is not None:
        assert sp.host_spans() == (n_host, host_bytes)
    assert sp.kernel_ms() > 0


@pytest.mark.parametrize("encoder", ENCODERS)
@pytest.mark.parametrize("kind", ["hostile", "ascii", "non_ascii"])
def test_fuzz_one_mib(splitters, encoder, kind):
    sp = splitters[encoder]
    sp.set_option("max_span", mbpe.SPLIT_MAX_SPAN)
    if kind == "non_ascii":
        data = S.random_text(43, 1 << 20, S.HOSTILE + S.ASCII, S.NON_ASCII, 0.08)
    else:
        data = S.random_text(41 if kind == "hostile" else 42, 1 << 20, S.HOSTILE if kind == "hostile" else S.ASCII)
    check(sp, encoder, data)
    assert (sp.host_spans()[0] > 0) == (kind == "non_ascii")


@pytest.mark.parametrize("encoder", ENCODERS)
def test_prefix_sweep(splitters, encoder):
    # one splitter over every length 0 .. 3 blocks, and around the first three tile multiples
    sp = splitters[encoder]
    sp.set_option("max_span", mbpe.SPLIT_MAX_SPAN)
    text = S.random_text(51, 3 * TILE + 8, S.HOSTILE)
    lengths = list(range(0, 3 * BLOCK + 1)) + [k * TILE + d for k in (1, 2, 3) for d in (-2, -1, 0, 1, 2)]
    for n in lengths:
        check(sp, encoder, text[:n])
    mixed = S.random_text(52, 3 * BLOCK + 8, S.HOSTILE, S.NON_ASCII, 0.08)
    for n in range(0, 3 * BLOCK + 1):
        if (mixed[n] & 0xC0) != 0x80:
            check(sp, encoder, mixed[:n])


@pytest.mark.parametrize("encoder", ENCODERS)
def test_no_sync_and_long_spans(splitters, encoder):
    sp = splitters[encoder]
    max_span = 256
    sp.set_option("max_span", max_span)
    try:
        for fill in (b"a", b"1", b" "):
            for n in (max_span - 1, max_span, max_span + 1, 3 * max_span + 5):
                check(sp, encoder, fill * n)
                # (no letter or digit before whitespace anywhere: the text is one span)
                assert sp.host_spans() == ((1, n) if n > max_span else (0, 0))
                # the run not block-aligned (gpt4 counts its groups of three digits from the start of the run), and a
                # run that is followed by more text
                check(sp, encoder, b"ab " + fill * n)
                check(sp, encoder, b"ab " + fill * n + b" cd\n\nef " + fill * n)
        check(sp, encoder, b"x" + b"1" * (max_span + 1))
        assert sp.host_spans() == (1, max_span + 2)
        check(sp, encoder, b"1" * max_span + b" 1")
        assert sp.host_spans() == (0, 0)
    finally:
        sp.set_option("max_span", mbpe.SPLIT_MAX_SPAN)


@pytest.mark.parametrize("encoder", ENCODERS)
def test_whitespace_and_newlines_across_block_edges(splitters, encoder):
    sp = splitters[encoder]
    sp.set_option("max_span", mbpe.SPLIT_MAX_SPAN)
    for lead in range(BLOCK - 6, BLOCK + 3):
        head = b"word " * 40
        head = head[:lead - 1] + b"a"                # a letter right before the run
        for ws in (b"   ", b" \n \n  ", b"\r\n\r\n", b"\t\t \x0b\x0c ", b" \r \n\t", b"\n", b"  \n"):
            for tail in (b"", b"x", b" x", b"'s", b"12345", b"!?\n\n", "été".encode(), b"\x00\x1c\x7f"):
                check(sp, encoder, head + ws + tail)
                check(sp, encoder, head + ws * 30 + tail)
    # trailing whitespace at the end of the text, and a text that ends in a host span
    for tail in (b" ", b"  ", b" \n", b"\n ", b"\t\t\t", b" " * 200):
        check(sp, encoder, b"the end" + tail)
        check(sp, encoder, b"x" * 300 + tail)
    check(sp, encoder, "one two café".encode())
    assert sp.host_spans()[0] == 1
    check(sp, encoder, "one two café  ".encode())
    check(sp, encoder, "中文 only".encode())
    check(sp, encoder, b"a " + "　".encode() * 50)


def bits_of(mask_tensor, n):
    return np.unpackbits(mask_tensor.cpu().numpy(), bitorder="little")[:n].astype(bool)


@pytest.mark.parametrize("encoder", ENCODERS)
def test_outputs(dev, splitters, encoder):
    sp = splitters[encoder]
    sp.set_option("max_span", mbpe.SPLIT_MAX_SPAN)
    data = np.frombuffer(read_data("taylorswift.txt"), dtype=np.uint8)
    n = len(data)
    want = mbpe.presplit(S.PATTERNS[encoder], data)
    n_chunks = len(want) - 1

    # the device mask equals the mask built from the offsets; the count is equal
    mask = torch.full((sp.mask_bytes(n),), 0xA5, dtype=torch.uint8, device=dev)
    got = sp.split(data, mask_ptr=mask.data_ptr())
    assert (got == want).all()
    assert (bits_of(mask, n) == S.end_mask_of(want, n)).all()
    assert not mask.cpu().numpy()[(n + 7) // 8:].any(), "bits beyond the text"
    assert sp.split(data, offsets=False) == n_chunks
    # (the mask the splitter keeps is what test_trainer_takes_the_mask loads)
    m_ptr, m_bytes, _ = sp.endmask()
    assert m_ptr and m_bytes == sp.mask_bytes(n)

    # a repeat call allocates nothing
    before = sp.alloc_count()
    sp.split(data, mask_ptr=mask.data_ptr())
    assert sp.alloc_count() == before

    # query mode; a cap too small reports the count, returns MBPE_ERR_ARG and writes nothing
    L = mbpe.lib()
    count = ctypes.c_uint64()
    off = np.full(n_chunks + 1, 7, dtype=np.uint64)
    mask.fill_(0xA5)
    rc = L.mbpe_splitter_split(sp._h, data.ctypes.data, n, 0, ctypes.c_void_p(mask.data_ptr()), off.ctypes.data,
                               n_chunks - 1, ctypes.byref(count))
    assert rc == mbpe.ERR_ARG and count.value == n_chunks
    assert (off == 7).all() and bool((mask == 0xA5).all())
    rc = L.mbpe_splitter_split(sp._h, data.ctypes.data, n, 0, None, off.ctypes.data, n_chunks, ctypes.byref(count))
    assert rc == 0 and (off == want).all()

    # device-resident text: the same result, the text untouched
    text = torch.from_numpy(data.copy()).to(dev)
    mask2 = torch.zeros(sp.mask_bytes(n), dtype=torch.uint8, device=dev)
    got = sp.split(text_ptr=text.data_ptr(), n_bytes=n, mask_ptr=mask2.data_ptr(), cap_chunks=n)
    assert (got == want).all()
    assert (bits_of(mask2, n) == S.end_mask_of(want, n)).all()
    assert sp.host_spans() == (109, 2142)
    assert (text.cpu().numpy() == data).all()


def test_custom_pattern_is_refused():
    h = ctypes.c_void_p()
    for pat in (b"", b"\\s+|\\S+", S.PATTERNS["gpt4"].encode() + b" "):
        assert mbpe.lib().mbpe_splitter_create(0, pat, ctypes.byref(h)) == mbpe.ERR_ARG
    with pytest.raises(mbpe.MbpeError) as e:
        mbpe.Tokenizer("\\s+|\\S+").train(read_data("sample.txt"), 300, device_split=True)
    assert e.value.code == mbpe.ERR_ARG
    with pytest.raises(mbpe.MbpeError) as e:
        mbpe.Tokenizer("").train(read_data("sample.txt"), 300, device_split=True)
    assert e.value.code == mbpe.ERR_ARG


@pytest.mark.parametrize("barrier", [None, 1])
def test_trainer_takes_the_mask(dev, splitters, barrier):
    data = np.frombuffer(read_data("taylorswift.txt"), dtype=np.uint8)
    sp = splitters["gpt4"]
    off = mbpe.presplit(S.PATTERNS["gpt4"], data)
    results = []
    for how in ("offsets", "mask, host text", "mask, device text"):
        with mbpe.Trainer(0) as tr:
            if barrier is not None:
                tr.set_option("chunk_barrier", barrier)
            if how == "offsets":
                tr.load_corpus(data, off)
            else:
                assert sp.split(data, offsets=False) == len(off) - 1
                m_ptr, _, t_ptr = sp.endmask()
                if how == "mask, host text":
                    tr.load_corpus_endmask(m_ptr, data=data)
                else:
                    tr.load_corpus_endmask(m_ptr, text_ptr=t_ptr, n_bytes=len(data), keep=sp)
            assert tr.stats()["n_chunks"] == len(off) - 1
            table = tr.pair_count_u8()
            tr.train_begin(300)
            tr.train_steps(300 - 256)
            merges, counts = tr.train_result()
            results.append((table, merges, counts))
    for table, merges, counts in results[1:]:
        assert (table == results[0][0]).all()
        assert merges.tolist() == results[0][1].tolist() and counts.tolist() == results[0][2].tolist()
    assert len(results[0][1]) == 300 - 256


@pytest.mark.parametrize("name", ["shakespeare_gpt4_lexical_512", "taylorswift_gpt4_lexical_512",
                                  "taylorswift_gpt2_lexical_512", "taylorswift_gpt4_first_512"])
def test_tokenizer_train_device_split_reproduces_the_golden_model(name):
    text, encoder, tie, _ = name.split("_")
    pat = S.PATTERNS[encoder]
    tok = mbpe.Tokenizer(pat)
    tok.train(read_data(text + ".txt"), 512, conflict_resolution=1 if tie == "lexical" else 0, device_split=True)
    assert O.model_bytes(pat, tok.merges()) == read_golden(name + ".model")


def test_cli_device_split(tmp_path):
    model = tmp_path / "m"
    r = subprocess.run([CLI, "-t", "-i", os.path.join(GOLDEN, "data", "taylorswift.txt"), "-m", str(model), "-c", "lexical",
                        "-v", "--device-split"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Split input text into 46196 chunks" in r.stdout
    assert model.read_bytes() == read_golden("taylorswift_gpt4_lexical_512.model")
