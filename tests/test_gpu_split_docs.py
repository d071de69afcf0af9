"""mbpe_splitter_split_docs on the device against the truth of tests/split_docs_cases.py (every part of every document
split on its own by mbpe_presplit; ranges from a Python restatement of split_on_special): random strings as documents,
the named edge cases, taylorswift.txt cut into documents with <|endoftext|> between some of them; host and device text;
max_span 1 and 64, so that spans which end at a cut take the host path too.  Then the old call against the new one,
allocation counts, and the error rules."""
import numpy as np
import pytest

import mbpe
import split_cases as S
import split_docs_cases as D
from conftest import read_data

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

ENCODERS = ["gpt2", "gpt4"]


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


_TRUTH = {}


def truth_of(encoder, key, blob, off, names):
    if (encoder, key) not in _TRUTH:
        _TRUTH[(encoder, key)] = D.truth(S.PATTERNS[encoder], blob, off, names)
    return _TRUTH[(encoder, key)]


def run(sp, dev, blob, off, names, on_device):
    """-> (bool[n] end mask read back from the device, n_chunks, ranges)."""
    blob = np.ascontiguousarray(blob, dtype=np.uint8)
    n = len(blob)
    mask_t = torch.zeros(mbpe.Splitter.mask_bytes(n), dtype=torch.uint8, device=dev)
    text_t = torch.from_numpy(blob.copy()).to(dev) if on_device and n else None
    torch.cuda.synchronize()
    if text_t is not None:
        n_chunks, ranges = sp.split_docs(doc_off=off, names=names, mask_ptr=mask_t.data_ptr(), text_ptr=text_t.data_ptr(),
                                         n_bytes=n)
    else:
        n_chunks, ranges = sp.split_docs(blob, off, names, mask_ptr=mask_t.data_ptr())
    raw = mask_t.cpu().numpy()
    bits = np.unpackbits(raw, bitorder="little")
    assert not bits[n:].any(), "end bits beyond the text"
    return bits[:n].astype(bool), n_chunks, ranges


def check(sp, dev, encoder, blob, off, names, on_device, truth=None):
    want, want_ranges, _ = truth if truth is not None else D.truth(S.PATTERNS[encoder], blob, off, names)
    got, n_chunks, ranges = run(sp, dev, blob, off, names, on_device)
    wrong = np.flatnonzero(got != want)
    assert len(wrong) == 0, "%s: %d chunk ends differ, first at byte %d" % (encoder, len(wrong), wrong[0])
    assert n_chunks == int(want.sum())
    assert ranges.tolist() == want_ranges.tolist()


@pytest.mark.parametrize("encoder", ENCODERS)
@pytest.mark.parametrize("on_device,max_span", [(False, mbpe.SPLIT_MAX_SPAN), (False, 64), (False, 1),
                                                (True, mbpe.SPLIT_MAX_SPAN), (True, 1)])
def test_random_strings_as_documents(splitters, dev, encoder, on_device, max_span):
    # 200,000 strings, about 4 MiB: hundreds of walk tiles, cuts on every residue mod 16 and mod 64
    blob, off = D.string_sets()
    sp = splitters[encoder]
    sp.set_option("max_span", max_span)
    try:
        check(sp, dev, encoder, blob, off, [], on_device, truth_of(encoder, "strings", blob, off, []))
        assert sp.host_spans()[0] > 1000
    finally:
        sp.set_option("max_span", mbpe.SPLIT_MAX_SPAN)


@pytest.mark.parametrize("encoder", ENCODERS)
@pytest.mark.parametrize("on_device", [False, True])
def test_random_strings_with_names(splitters, dev, encoder, on_device):
    blob, off = D.string_sets(30000)
    names = [b"sd", b" t", b"'", b"\n\n", "é".encode(), b"sdm"]
    sp = splitters[encoder]
    check(sp, dev, encoder, blob, off, names, on_device, truth_of(encoder, "names", blob, off, names))
    assert sp.find_ms() > 0 and sp.kernel_ms() >= sp.find_ms()


@pytest.mark.parametrize("encoder", ENCODERS)
@pytest.mark.parametrize("max_span", [mbpe.SPLIT_MAX_SPAN, 1])
def test_named_cases(splitters, dev, encoder, max_span):
    sp = splitters[encoder]
    sp.set_option("max_span", max_span)
    try:
        for cid, docs, names in D.NAMED:
            blob, off = D.join(docs)
            for on_device in (False, True):
                try:
                    check(sp, dev, encoder, blob, off, names, on_device)
                except AssertionError as e:
                    raise AssertionError("%s (device text %s): %s" % (cid, on_device, e))
    finally:
        sp.set_option("max_span", mbpe.SPLIT_MAX_SPAN)


def swift_documents():
    """taylorswift.txt cut into documents at 3,000 random character boundaries, <|endoftext|> inserted at 1,000 of them."""
    data = read_data("taylorswift.txt")
    rng = np.random.default_rng(77)
    arr = np.frombuffer(data, dtype=np.uint8)
    bounds = np.flatnonzero((arr & 0xC0) != 0x80)
    cuts = np.sort(rng.choice(bounds[1:], 3000, replace=False))
    eot = set(rng.choice(cuts, 1000, replace=False).tolist())
    docs, last = [], 0
    for c in cuts.tolist() + [len(data)]:
        docs.append(data[last:c] + (D.E if c in eot else b""))
        last = c
    return D.join(docs)


@pytest.mark.parametrize("encoder", ENCODERS)
@pytest.mark.parametrize("on_device,max_span", [(False, mbpe.SPLIT_MAX_SPAN), (True, mbpe.SPLIT_MAX_SPAN), (False, 64),
                                                (True, 1)])
def test_taylorswift_cut_into_documents(splitters, dev, encoder, on_device, max_span):
    blob, off = swift_documents()
    sp = splitters[encoder]
    sp.set_option("max_span", max_span)
    try:
        t = truth_of(encoder, "swift", blob, off, [D.E])
        check(sp, dev, encoder, blob, off, [D.E], on_device, t)
        assert len(t[1]) == 1000 and (t[1][:, 2] == 0).all()
        assert sp.host_spans()[0] > 0                      # non-ASCII characters: host spans, some of them end at cuts
    finally:
        sp.set_option("max_span", mbpe.SPLIT_MAX_SPAN)


@pytest.mark.parametrize("encoder", ENCODERS)
def test_one_document_without_names_is_the_old_call(splitters, dev, encoder):
    sp = splitters[encoder]
    for name in ("taylorswift.txt", "specialtokensample.txt"):
        data = np.frombuffer(read_data(name), dtype=np.uint8)
        off = sp.split(data, cap_chunks=len(data))
        assert (off == mbpe.presplit(S.PATTERNS[encoder], data)).all()
        got, n_chunks, ranges = run(sp, dev, data, [0, len(data)], [], False)
        assert n_chunks == len(off) - 1 and len(ranges) == 0
        assert (got == S.end_mask_of(off, len(data))).all()
    # repeat calls of no larger size allocate nothing, whichever of the two calls they are
    blob, off = swift_documents()
    mask_t = torch.zeros(mbpe.Splitter.mask_bytes(len(blob)), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    sp.split_docs(blob, off, [D.E], mask_ptr=mask_t.data_ptr())
    sp.split(blob, offsets=False)
    before = sp.alloc_count()
    for _ in range(2):
        sp.split_docs(blob, off, [D.E], mask_ptr=mask_t.data_ptr())
        sp.split(blob, offsets=False)
        sp.split_docs(b"some words here " * 60, [0, 10, 960], [D.E, b"x"])
    assert sp.alloc_count() == before


def test_empty_inputs(splitters, dev):
    sp = splitters["gpt4"]
    assert sp.split_docs(b"", [0], [D.E])[0] == 0
    assert sp.split_docs(b"", [0, 0, 0], [])[0] == 0
    n_chunks, ranges = sp.split_docs(b"", np.zeros(1, dtype=np.uint64), [])
    assert n_chunks == 0 and len(ranges) == 0


def test_errors(splitters, dev):
    sp = splitters["gpt4"]
    text = b"one <e> two"
    with pytest.raises(mbpe.MbpeError) as e:
        sp.split_docs(text, [0, len(text)], [b"n%03d" % k for k in range(257)])
    assert e.value.code == mbpe.ERR_ARG
    assert sp.split_docs(text, [0, len(text)], [b"n%03d" % k for k in range(256)])[0] > 0
    with pytest.raises(mbpe.MbpeError) as e:
        sp.split_docs(text, [0, len(text)], [b"x" * 16385])
    assert e.value.code == mbpe.ERR_ARG
    with pytest.raises(mbpe.MbpeError) as e:
        sp.split_docs(text, [0, 7, 5, len(text)], [])
    assert e.value.code == mbpe.ERR_ARG
    with pytest.raises(mbpe.MbpeError) as e:
        sp.split_docs(text, [0, len(text) - 1], [])
    assert e.value.code == mbpe.ERR_ARG
    # too little room for the ranges: the count comes back, the caller's mask stays as it was
    text = b"a<e>b<e>c"
    mask_t = torch.full((mbpe.Splitter.mask_bytes(len(text)),), 0xAB, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    with pytest.raises(mbpe.MbpeError) as e:
        sp.split_docs(text, [0, len(text)], [b"<e>"], mask_ptr=mask_t.data_ptr(), cap_ranges=1)
    assert e.value.code == mbpe.ERR_ARG and sp.n_ranges == 2
    assert (mask_t.cpu().numpy() == 0xAB).all()
    n_chunks, ranges = sp.split_docs(text, [0, len(text)], [b"<e>"], cap_ranges=2)
    assert n_chunks == 5 and ranges.tolist() == [[1, 3, 0], [5, 3, 0]]
    # invalid UTF-8 inside a host span: PCRE2's match runs over the span's end
    bad = b"ab \xe4a cd ef"
    with pytest.raises(mbpe.MbpeError) as e:
        sp.split_docs(bad, [0, 9, len(bad)], [b"cd"], mask_ptr=mask_t.data_ptr())
    assert e.value.code == mbpe.ERR_SPLIT_GAP
    assert (mask_t.cpu().numpy() == 0xAB).all()
    with pytest.raises(mbpe.MbpeError):
        sp.endmask()                                           # no mask of a failed call
    assert sp.split_docs(text, [0, len(text)], [b"<e>"])[0] == 5   # the splitter stays usable
