"""One encoder, many calls: the steps, schedules, references and the checker of tests/test_gpu_encoder_history.py and
tests/test_history_cases_cpu.py.  Plain Python and numpy: nothing here touches a device or libmbpe.so.

The property: the result of an encoder call is a function of that call's arguments and the settings in force, never of
the calls made before it (the count table, which accumulates until it is reset, is the one exception).

A Step names the settings in force, the call (one of eight route classes), the input from a fixed pool and the form of
the output.  expected(step) composes what the call must give from the references the suite already has -- each a
restatement of a rule of include/mbpe.h in Python -- and depends on the step alone.  check(step, got, want) compares
whole arrays, exactly.  A Schedule is a list of steps for ONE encoder: eight hand-made ones that go large -> small ->
large around the buffers that are kept, borrowed and reused, and constructed ones whose route classes follow an
Eulerian circuit of the complete directed graph on the eight classes, so that every class follows every class once."""
import copy
import dataclasses
import functools
import random
import re

import numpy as np

import byteoff_cases as B
import dedup_cases as DD
import dropout_cases as D
import encode_cases as E
import encode_rank_cases as R
import fim_cases as F
import fit_cases as FIT
import hist_cases as H
import mlm_cases as M
import window_cases as W
from conftest import read_data, read_golden

OK, ERR_ARG, ERR_VOCAB, ERR_STATE, ERR_OOM = 0, -1, -4, -5, -6          # MBPE_OK, MBPE_ERR_* (include/mbpe.h)
END = 0x80000000                        # bit 31 of a 32-bit token on the device: last token of its chunk
GUARD = 64                              # elements every device output is longer than it needs to be
SENTINEL = {1: 0xA5, 2: 0xA5A5, 4: 0xA5A5A5A5, 8: 0xA5A5A5A5A5A5A5A5}    # by element size; no expected value equals one
ROUTES = ("plain", "byteoff", "endmask", "pack", "aux", "windows", "fit", "count")
BATCH = ("pack", "aux", "windows", "fit")
PAD, BOS, EOS = 3, 1, 2
IGNORE = {16: 65000, 32: -100}
SMALL_LENGTHS = (0, 1, 2, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025)
SMALL = tuple("s%d" % n for n in SMALL_LENGTHS)
MODEL = "taylorswift_gpt4_first_512"


# ---- the merges table and the pool of inputs --------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def merges():
    """The golden model's merges, then those pairs of encode_cases.nul_merges() that keep the table one
    mbpe_merges_check accepts (both sides below the pair's own id, no pair twice): pairs over the bytes a NUL marker is
    written with and over the small ids the markers of the pool stand for."""
    out = [tuple(int(v) for v in m) for m in B.parse_model(read_golden(MODEL + ".model"))[1]]
    seen = set(out)
    for a, b in E.nul_merges().tolist():
        k = len(out)
        if a < 256 + k and b < 256 + k and (a, b) not in seen:
            out.append((a, b))
            seen.add((a, b))
    m = np.array(out, dtype=np.uint32)
    m.setflags(write=False)
    return m


def n_table_ids():
    return 256 + len(merges())


@dataclasses.dataclass(frozen=True)
class Input:
    name: str
    data: bytes
    chunk_off: np.ndarray               # uint64[n_chunks + 1]; empty chunks allowed
    doc_chunk_off: np.ndarray           # uint64[n_docs + 1]: chunk indices

    @property
    def n_docs(self):
        return len(self.doc_chunk_off) - 1

    @property
    def doc_off(self):
        """byte offsets of the documents: what the endmask calls take"""
        return self.chunk_off[self.doc_chunk_off.astype(np.int64)]

    def chunks(self):
        off = self.chunk_off.astype(np.int64).tolist()
        return [self.data[a:b] for a, b in zip(off[:-1], off[1:])]


def split_words(b):
    """A simple split that tiles the text: a word or a number with the blank before it, blanks, anything else."""
    parts = re.findall(rb" ?[A-Za-z]+| ?[0-9]+|\s+|[^\sA-Za-z0-9]+", b)
    assert b"".join(parts) == b
    return parts


MARKERS = (b"\x000", b"\x0012", b"\x00300", b"\x00 7", b"\x00+49", b"\x0012abc", b"\x007\x0012", b"\x0000012")
NOT_MARKERS = (b"\x00abc", b"\x00", b"\x00+", b"\x00 ")                # NUL-led, yet no number: they stay bytes


def _make(name, pieces, doc_every, empty_doc_every=0):
    off = np.zeros(len(pieces) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(p) for p in pieces], dtype=np.uint64)
    n = len(pieces)
    if doc_every:
        bounds = []
        for k, c in enumerate(range(0, n, doc_every)):
            bounds.append(c)
            if empty_doc_every and k % empty_doc_every == 1:
                bounds.append(c)                                     # an empty document
        bounds += [n, n] if empty_doc_every else [n]                  # (and one at the very end)
    else:
        bounds = [0, n]
    docs = np.array(bounds, dtype=np.uint64)
    for a in (off, docs):
        a.setflags(write=False)
    return Input(name, b"".join(pieces), off, docs)


@functools.lru_cache(maxsize=None)
def pool():
    """name -> Input.  One merges table for all of it."""
    ts = read_data("taylorswift.txt")
    out = {}
    # large: empty chunks first, last and three in a row; 300 NUL markers among the words from the start on; 1,100
    # chunks of one byte in a row; 600 equal and 600 distinct chunks; one chunk longer than the deduper's limit
    pieces = [b""]
    k = 0
    words = split_words(ts[:11000])
    every = len(words) // 300
    assert every >= 2
    for i, w in enumerate(words):
        pieces.append(w)
        if i % every == every // 2 and k < 300:
            pieces.append(MARKERS[k % len(MARKERS)])
            k += 1
            if k % 37 == 0:
                pieces.append(NOT_MARKERS[(k // 37) % len(NOT_MARKERS)])
    assert k == 300
    pieces += [bytes([c]) for c in ts[11000:12100]]
    pieces += [b"", b"", b""]
    pieces += [b" the"] * 600
    pieces += [b" %04d" % i for i in range(600)]
    pieces.append(ts[12100:12700])
    pieces += split_words(ts[12700:12700 + 18500])
    pieces.append(b"")
    out["large"] = _make("large", pieces, 8, 50)
    # medium: the same kinds, fewer of each
    pieces = [b""]
    for i, w in enumerate(split_words(ts[40000:42900])):
        pieces.append(w)
        if i in (3, 200, 400):
            pieces.append(MARKERS[i % len(MARKERS)])
    pieces += [bytes([c]) for c in ts[43000:43040]] + [b"", b""] + [b" the"] * 10 + [b""]
    out["medium"] = _make("medium", pieces, 20, 7)
    # ones: every byte a chunk of its own -- the end mask is all ones and the chunk ends need a list of their own
    out["ones"] = _make("ones", [bytes([c]) for c in ts[50000:90000]], 32)
    # small: one chunk where the length is a multiple of 32, else words (the last end is then inside a mask word)
    for n in SMALL_LENGTHS:
        text = ts[30000:30000 + n]
        out["s%d" % n] = _make("s%d" % n, [text] if n % 32 == 0 else split_words(text), 0)
    for inp in out.values():
        assert b"\x00" not in inp.data or inp.name in ("large", "medium")
    return out


@functools.lru_cache(maxsize=None)
def nul_singles(name):
    """The chunks of an input that the NUL rule makes one token, as rows (start, len, id): what a caller of the endmask
    calls has to say, since there no chunk is parsed for a number."""
    inp = pool()[name]
    off = inp.chunk_off.astype(np.int64).tolist()
    rows = []
    for a, b in zip(off[:-1], off[1:]):
        sid = B.stoi_single(inp.data[a:b]) if b > a else None
        if sid is not None:
            rows.append((a, b - a, sid))
    return tuple(rows)


def end_mask(inp):
    """The end mask of the header's layout: 2 * ceil(n / 16) + 16 bytes, nothing set at or beyond n_bytes."""
    return DD.end_mask(inp.chunk_off, len(inp.data))


# ---- steps ----------------------------------------------------------------------------------------------------------------

DEFAULTS = dict(order="greedy", dropout=None, dedup=False, dedup_max=256, piece_bytes=0, fim=None, mlm=None, count_ids=0)
FIM_ONE = F.spec(rate=F.ONE, spm=F.ONE // 2, seed=9, doc_base=5)
FIM_HALF = F.spec(rate=F.ONE // 2, spm=F.ONE // 3, seed=4, doc_base=1 << 40, min_tokens=2, max_tokens=400)
MLM_WORD = M.spec(M.threshold(0.4), seed=11, doc_base=3, mask_id=600, vocab_n=500, whole_word=1, protect=(32, 10))
MLM_TOKEN = M.spec(M.threshold(0.3), seed=2, mask_id=601, vocab_n=256, whole_word=0, protect=(101,))
PACK_DEFAULT = dict(seq_len=24, layout="padded", pad=PAD, bos=None, eos=EOS, pad_left=False, trunc_left=False, stride=5,
                    score_once=True)


@dataclasses.dataclass
class Step:
    route: str                          # one of ROUTES
    inp: str                            # a name of pool()
    set: dict                           # EVERY setting in force at the call (the runner applies what differs)
    endmask: bool = False               # the call's endmask form (always for the route "endmask")
    text: str = "host"                  # "host", "dev", "dev1" (device memory, one byte behind a 16-byte boundary)
    out: str = "host"                   # "host", "dev"
    bits: int = 32                      # 16, 32
    cap: str = "n"                      # "n": exactly what is needed; "query"; "short": one less, which is refused
    offsets: bool = False               # the chunks' token offsets (flat calls on a text with chunk_off)
    docs: bool = True                   # the documents' offsets (flat endmask calls)
    byteoff: bool = False               # token byte offsets (the route "byteoff"; flat endmask calls)
    singles: object = "auto"            # endmask calls: "auto" (nul_singles of the input), or rows (start, len, id)
    pack: dict = None                   # batch calls: see PACK_DEFAULT
    reset: bool = False                 # count: reset_counts() first
    repeat: int = 1                     # count

    def __post_init__(self):
        assert self.route in ROUTES and self.inp in pool() and sorted(self.set) == sorted(DEFAULTS)
        if self.route == "endmask":
            self.endmask = True
        if self.route == "byteoff":
            self.byteoff = True
        if self.endmask:
            self.text = "dev"
        if self.route in BATCH:
            self.pack = dict(PACK_DEFAULT, **(self.pack or {}))

    def describe(self):
        changed = {k: v for k, v in self.set.items() if v != DEFAULTS[k]}
        for k in ("fim", "mlm"):
            if k in changed:
                changed[k] = "on(seed %d)" % changed[k]["seed"]
        what = [self.route + ("/endmask" if self.endmask and self.route != "endmask" else ""), self.inp,
                "text=" + self.text, "out=" + self.out, "bits=%d" % self.bits, "cap=" + self.cap]
        what += [k for k in ("offsets", "byteoff", "reset") if getattr(self, k)]
        if self.endmask:
            what.append("singles=" + (self.singles if isinstance(self.singles, str) else repr(list(self.singles))))
            what.append("docs" if self.docs else "no docs")
        if self.pack:
            what.append("pack=%r" % {k: v for k, v in self.pack.items() if v != PACK_DEFAULT.get(k)})
        return "%s  settings: %r" % (" ".join(what), changed)


@dataclasses.dataclass
class Schedule:
    name: str
    doc: str
    steps: list


class _Builder:
    """Steps with the settings carried from one to the next: set() changes what is in force from the next step on."""

    def __init__(self, name, doc):
        self.sched, self.cur = Schedule(name, doc, []), dict(DEFAULTS)

    def set(self, **kw):
        assert set(kw) <= set(DEFAULTS)
        self.cur.update(kw)
        return self

    def add(self, route, inp, **kw):
        self.sched.steps.append(Step(route, inp, dict(self.cur), **kw))
        return self


# ---- the references ---------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _lookup():
    return {(int(a), int(b)): 256 + k for k, (a, b) in enumerate(merges().tolist())}


_CHUNK = {}


def _chunk_tokens(chunk, rank):
    """byteoff_cases.encode_chunk of one chunk at offset 0, remembered: a text repeats its words"""
    v = _CHUNK.get((chunk, rank))
    if v is None:
        v = _CHUNK[(chunk, rank)] = tuple(tuple(t) for t in B.encode_chunk(chunk, 0, _lookup(), rank))
    return v


def _singles_key(step):
    """"nul": the NUL rule (calls with chunk_off); else the rows (start, len, id) an endmask call is given"""
    if not step.endmask:
        return "nul"
    return nul_singles(step.inp) if step.singles == "auto" else tuple(tuple(int(v) for v in r) for r in step.singles)


@functools.lru_cache(maxsize=None)
def stream(name, order, dropout, singles):
    """The tokens of an input -> (ids uint32, end: True on the last token of a chunk, pos: the byte every token starts
    at), read-only.  Without dropout: byteoff_cases.encode_chunk chunk by chunk, in either order; with it (p = 0
    included): dropout_cases.reference over the whole text.  singles "nul": a NUL-led chunk with a number is one token;
    rows (start, len, id): those ranges are, and no chunk is parsed."""
    inp = pool()[name]
    return stream_of_text(inp.data, inp.chunk_off, order, dropout, singles)


def stream_of_text(data, chunk_off, order, dropout, singles):
    """stream() of any text with its chunk offsets"""
    if dropout is not None:
        assert order == "rank"
        tok, end, pos, _ = D.reference(data, chunk_off, merges(), dropout[1], D.threshold_of(dropout[0]),
                                       None if singles == "nul" else list(singles))
        out = (tok.astype(np.uint32), end.astype(bool), pos.astype(np.uint64))
    else:
        given = {} if singles == "nul" else {s: (ln, i) for s, ln, i in singles}
        off = np.asarray(chunk_off).astype(np.int64).tolist()
        ids, pos, end = [], [], []
        for a, b in zip(off[:-1], off[1:]):
            if b == a:
                continue
            if a in given:
                assert given[a][0] == b - a, "a single is a whole chunk"
                toks = ((given[a][1], 0, b - a),)
            else:
                # (an endmask call parses nothing: the pool gives it every NUL-led number as a single)
                assert singles == "nul" or B.stoi_single(data[a:b]) is None
                toks = _chunk_tokens(data[a:b], order == "rank")
            ids += [t[0] for t in toks]
            pos += [a + t[1] for t in toks]
            end += [False] * (len(toks) - 1) + [True]
        out = (np.array(ids, dtype=np.uint32), np.array(end, dtype=bool), np.array(pos, dtype=np.uint64))
    for a in out:
        a.setflags(write=False)
    return out


def _dropout_key(step):
    """(p, seed), or None where it plays no part: p = 0 in the greedy order is the greedy order"""
    return step.set["dropout"] if _threshold(step) or step.set["order"] == "rank" else None


def _stream_of(step):
    return stream(step.inp, step.set["order"], _dropout_key(step), _singles_key(step))


@functools.lru_cache(maxsize=None)
def _chunk_tok_off(name, order, dropout, singles):
    inp = pool()[name]
    off = R.chunk_tok_off(stream(name, order, dropout, singles)[1], len(inp.data), inp.chunk_off)
    off.setflags(write=False)
    return off


def _doc_tok_off(step):
    inp = pool()[step.inp]
    ctoff = _chunk_tok_off(step.inp, step.set["order"], _dropout_key(step), _singles_key(step))
    return ctoff[inp.doc_chunk_off.astype(np.int64)].astype(np.uint64)


@functools.lru_cache(maxsize=None)
def dedup_counts(name, max_chunk_bytes):
    """(chunks the deduper keeps, unique chunks, their bytes): dedup_cases.dedup of the chunks that are not empty"""
    chunks = [c for c in pool()[name].chunks() if c]
    uniq, _, _ = DD.dedup(chunks, max_chunk_bytes)
    return len(chunks), len(uniq), sum(len(c) for c in uniq)


def _threshold(step):
    return 0 if step.set["dropout"] is None else D.threshold_of(step.set["dropout"][0])


def refusal(step):
    """The error code a step must be refused with, or None.  Every one of them is a refusal the header documents as
    leaving the encoder usable; the order is that of the header: what is checked before the device is touched, then
    the ids, then the pieces, and the cap after the passes."""
    s = step.set
    inp = pool()[step.inp]
    if _threshold(step) and s["order"] == "greedy":
        return ERR_ARG                                               # dropout is defined on the rank order alone
    if _threshold(step) and s["dedup"]:
        return ERR_ARG
    if step.byteoff and s["dedup"] and step.cap != "query":
        return ERR_ARG
    if step.route in BATCH:
        if s["fim"] is not None and s["mlm"] is not None:
            return ERR_ARG
        if s["mlm"] is not None and s["mlm"]["whole_word"] and step.bits == 16:
            return ERR_ARG
    if step.endmask and step.bits == 16 and any(i >= 65536 for _, _, i in _singles_key(step)):
        return ERR_VOCAB
    if s["piece_bytes"] and len(inp.data):
        if s["dedup"]:
            too_long = dedup_counts(step.inp, s["dedup_max"])[2] > s["piece_bytes"]
        elif step.endmask:
            too_long = len(inp.data) > s["piece_bytes"]
        else:
            too_long = int(np.diff(inp.chunk_off.astype(np.int64)).max()) > s["piece_bytes"]
        if too_long:
            return ERR_OOM
    if step.cap == "short":
        return ERR_ARG
    return None


def _ids_dtype(bits):
    return np.uint16 if bits == 16 else np.uint32


def _label_dtype(bits):
    return np.uint16 if bits == 16 else np.int32


def _rows(rows, seq_len, dtype):
    a = np.array(rows, dtype=np.int64).reshape(len(rows), seq_len)
    return a.astype(dtype)


def _stage(step, docs, ends, off):
    """The stage between encode and pack -> (documents as lists of ids, targets per document or None, fim modes, cuts,
    offsets after it)."""
    s = step.set
    n_docs = len(docs)
    modes, cuts, tgt = [0] * n_docs, [[0, 0]] * n_docs, None
    if s["fim"] is not None:
        new_off, modes, cuts = F.ref_plan([len(d) for d in docs], s["fim"])
        docs = F.ref_apply(docs, s["fim"])
        off = np.array(new_off, dtype=np.uint64)
        assert [len(d) for d in docs] == np.diff(off.astype(np.int64)).tolist()
    elif s["mlm"] is not None:
        ids = [t for d in docs for t in d]
        new, flat_tgt = M.ref_apply(s["mlm"], ids, ends.tolist(), off)
        o = off.astype(np.int64).tolist()
        docs = [new[a:b] for a, b in zip(o[:-1], o[1:])]
        tgt = flat_tgt
    return docs, tgt, np.array(modes, dtype=np.uint8), np.array(cuts, dtype=np.uint64).reshape(n_docs, 2), off


def _run_boundaries(seg, lengths, by_rows):
    """The boundaries of the maximal runs of equal (row, seg): over the stream's cells of a PACKED matrix, or -- by_rows,
    the fit layout -- over the whole matrix, pad runs included (fit_cases.cu_of)."""
    if by_rows:
        return FIT.cu_of({"seg": seg.tolist()}, seg.shape[1]) if seg.shape[0] else ([0], 0)
    from test_gpu_pack_aux import run_boundaries
    cu = run_boundaries(seg, lengths)
    return cu, max([b - a for a, b in zip(cu[:-1], cu[1:])], default=0)


def _expected_batch(step):
    from test_gpu_pack import ref_pack
    from test_gpu_pack_aux import ref_aux
    tok, ends, _ = _stream_of(step)
    return matrices(step, tok, ends, _doc_tok_off(step))


def matrices(step, tok, ends, off):
    """What a batch call makes of a token stream with its end flags and the documents' token offsets: the stage, then
    the packer of the step's route."""
    from test_gpu_pack import ref_pack
    from test_gpu_pack_aux import ref_aux
    p, bits = step.pack, step.bits
    o = off.astype(np.int64).tolist()
    docs = [tok[a:b].tolist() for a, b in zip(o[:-1], o[1:])]
    docs, tgt, modes, cuts, off = _stage(step, docs, ends, off)
    o = off.astype(np.int64).tolist()
    L = np.diff(np.array(o, dtype=np.int64))
    flat = np.array([t for d in docs for t in d], dtype=np.uint32)
    S, bos, eos, ign, PAD = p["seq_len"], p["bos"], p["eos"], IGNORE[bits], p["pad"]
    nb, ne = int(bos is not None), int(eos is not None)
    keep = S - nb - ne
    want = {"error": OK, "n_tokens": len(tok), "fim_info": (modes, cuts)}
    if step.route != "pack":
        want["doc_tok_off"] = off
    if step.route == "pack":
        ids, lengths = ref_pack(flat, off, S, p["layout"], bits, PAD, bos, eos, p["pad_left"], p["trunc_left"])
        m = {"ids": ids, "lengths": lengths}
        tok_of = None
    elif step.route == "aux":
        ids, lengths, labels, pos, seg = ref_aux(flat, off, S, p["layout"], bits, PAD, bos, eos, p["pad_left"],
                                                 p["trunc_left"], ign)
        m = {"ids": ids, "lengths": lengths, "labels": labels.view(_label_dtype(bits)), "positions": pos, "segments": seg}
        if p["layout"] == "packed":
            cu, longest = _run_boundaries(seg, lengths, False)
            want["cu_seqlens"], want["max_seqlen"] = np.array(cu, dtype=np.int32), longest

            def tok_of(r, c, d, k):
                return k - nb if nb <= k < nb + L[d] else None
        else:
            def tok_of(r, c, d, k):
                body = min(int(L[d]), keep)
                first = int(L[d]) - body if p["trunc_left"] else 0
                return first + k - nb if nb <= k < nb + body else None
    elif step.route == "windows":
        ref = W.ref_windows(docs, S, p["stride"], bos, eos, PAD, ign, p["score_once"])
        n = len(ref["len"])
        m = {"ids": _rows(ref["ids"], S, _ids_dtype(bits)), "lengths": np.array(ref["len"], dtype=np.uint32),
             "labels": _rows(ref["labels"], S, _label_dtype(bits)), "positions": _rows(ref["pos"], S, np.uint32),
             "segments": _rows(ref["seg"], S, np.uint32), "row_doc": np.array(ref["row_doc"], dtype=np.uint32),
             "row_tok0": np.array(ref["row_tok0"], dtype=np.uint64)}
        assert n == len(m["ids"])
        tok0 = ref["row_tok0"]

        def tok_of(r, c, d, k):
            a = int(tok0[r])
            body = min(keep, int(L[d]) - a)
            if not nb <= k < nb + body:
                return None
            if p["score_once"] and a > 0 and k < nb + p["stride"]:
                return None                                          # a cell the window before held too
            return a + k - nb
    else:
        ref = FIT.ref_fit(docs, S, bos, eos, PAD, ign)
        n = len(ref["len"])
        seg = _rows(ref["seg"], S, np.uint32)
        m = {"ids": _rows(ref["ids"], S, _ids_dtype(bits)), "lengths": np.array(ref["len"], dtype=np.uint32),
             "labels": _rows(ref["labels"], S, _label_dtype(bits)), "positions": _rows(ref["pos"], S, np.uint32),
             "segments": seg, "doc_row": np.array(ref["doc_row"], dtype=np.uint64),
             "doc_col": np.array(ref["doc_col"], dtype=np.uint32)}
        cu, longest = _run_boundaries(seg, m["lengths"], True)
        want["cu_seqlens"], want["max_seqlen"] = np.array(cu, dtype=np.int32), longest

        def tok_of(r, c, d, k):
            return k - nb if nb <= k < nb + L[d] else None
    if tgt is not None and "labels" in m:
        lab = M.ref_labels({"segments": m["segments"], "positions": m["positions"]}, tgt, o, nb, ne, ign, tok_of)
        m["labels"] = lab.astype(_label_dtype(bits))
    want["n_rows"] = len(m["ids"])
    if step.cap != "query":
        want.update(m)
    return want


_EXPECTED = {}


def expected(step):
    """What the call of a step must give, from the step alone -> dict (remembered per step: treat it as read-only).
    "error": the code; on MBPE_OK the outputs by name, on a refused cap the count that is still reported."""
    key = repr(step)
    if key not in _EXPECTED:
        _EXPECTED[key] = _expected(step)
    return _EXPECTED[key]


def _expected(step):
    inp = pool()[step.inp]
    err = refusal(step)
    s = step.set
    if err is not None:
        want = {"error": err}
        only_cap = err == ERR_ARG and step.cap == "short" and refusal(dataclasses.replace(step, cap="n")) is None
        if only_cap and step.route in BATCH:
            ok = _expected_batch(dataclasses.replace(step, cap="n"))
            want["n_rows"], want["n_tokens"] = ok["n_rows"], ok["n_tokens"]
        elif only_cap:
            want["n_out"] = len(_stream_of(step)[0])
        return want
    if step.route in BATCH:
        want = _expected_batch(step)
    else:
        tok, ends, pos = _stream_of(step)
        n = len(tok)
        want = {"error": OK, "n_out": n}
        if step.route == "count":
            n_ids = max(n_table_ids(), s["count_ids"])
            counts, other = H.reference(tok, n_ids)
            want["delta"] = (counts * np.uint64(step.repeat), other * step.repeat, n * step.repeat)
        else:
            if step.cap != "query":
                if step.bits == 16:
                    want["tokens"] = tok.astype(np.uint16)
                elif step.out == "dev":
                    want["tokens"] = tok | (ends.astype(np.uint32) << np.uint32(31))
                else:
                    want["tokens"] = tok.copy()
                if step.byteoff:
                    want["byte_off"] = D.byte_offsets(pos, len(inp.data))
            if step.offsets and not step.endmask:
                want["chunk_tok_off"] = _chunk_tok_off(step.inp, s["order"], _dropout_key(step), "nul").astype(np.uint64)
            if step.endmask and step.docs:
                want["doc_tok_off"] = _doc_tok_off(step)
    # the route "dedup": what the deduper saw, or MBPE_ERR_STATE where the call did not go that way
    want["dedup_stats"] = dedup_counts(step.inp, s["dedup_max"]) if s["dedup"] else ERR_STATE
    if s["dedup"] and not len(inp.data):
        want["dedup_stats"] = (0, 0, 0)
    return want


# ---- the checker --------------------------------------------------------------------------------------------------------------

class Mismatch(AssertionError):
    pass


def _same(name, got, want):
    if isinstance(want, np.ndarray):
        if not isinstance(got, np.ndarray):
            return "%s: got %r, want an array" % (name, type(got))
        if got.dtype != want.dtype or got.shape != want.shape:
            return "%s: got %s%s, want %s%s" % (name, got.dtype, got.shape, want.dtype, want.shape)
        if not np.array_equal(got, want):
            at = tuple(int(v) for v in np.argwhere(got != want)[0])
            return "%s: %d elements differ, the first at %s: got %s, want %s" % (name, int((got != want).sum()), at,
                                                                                 got[at], want[at])
        return None
    if isinstance(want, tuple):
        if not isinstance(got, tuple) or len(got) != len(want):
            return "%s: got %r, want %r" % (name, got, want)
        for k, (g, w) in enumerate(zip(got, want)):
            bad = _same("%s[%d]" % (name, k), g, w)
            if bad:
                return bad
        return None
    return None if type(got) in (int, np.int64, np.uint64) and int(got) == int(want) else \
        "%s: got %r, want %r" % (name, got, want)


def check(step, got, want):
    """Exact, on whole arrays: the error code; dtype, shape and every element of everything `want` names; nothing in the
    `got` of a call that succeeded that `want` does not name; and every guard -- the sentinel behind each device
    output, or the whole buffer where a refused call may write nothing -- untouched.  Raises Mismatch."""
    bad = []
    for name, w in want.items():
        if name == "delta":
            continue                                                # (the judge turns it into "counts")
        if name not in got:
            bad.append("%s: missing" % name)
            continue
        b = _same(name, got[name], w)
        if b:
            bad.append(b)
    for name in got:
        if name not in want and name != "guards" and want["error"] == OK:
            bad.append("%s: not expected (%r)" % (name, type(got[name])))
    for name, arr in got.get("guards", {}).items():
        sent = SENTINEL[arr.dtype.itemsize]
        flat = arr.reshape(-1).view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[arr.dtype.itemsize])
        if not (flat == sent).all():
            at = int(np.flatnonzero(flat != sent)[0])
            bad.append("guard of %s: %d elements overwritten, the first at +%d (%#x)" % (
                name, int((flat != sent).sum()), at, int(flat[at])))
    if bad:
        raise Mismatch("; ".join(bad))


class CountTable:
    """What counts() must give: the sum of the references of the count steps since the last reset."""

    def __init__(self):
        self.table, self.other, self.total = None, 0, 0

    def add(self, step, want):
        """-> (counts, n_other, n_tokens) after the step"""
        n_ids = max(n_table_ids(), step.set["count_ids"])
        if step.reset or self.table is None:
            self.table, self.other, self.total = np.zeros(n_ids, dtype=np.uint64), 0, 0
        assert len(self.table) == n_ids, "count_ids changes only together with a reset"
        if want["error"] == OK:
            counts, other, total = want["delta"]
            self.table = self.table + counts
            self.other += other
            self.total += total
        return self.table.copy(), self.other, self.total


class Judge:
    """The checks of one schedule on one encoder: expected() per step, the count table summed since the last reset, and
    a failure message that names the schedule, the step and the three before it."""

    def __init__(self, sched):
        self.sched = sched
        self.counts = CountTable()

    def want(self, i):
        """expected() of step i; call it once per step, in order: the count steps add up"""
        step = self.sched.steps[i]
        want = dict(expected(step))
        if step.route == "count":
            want["counts"] = self.counts.add(step, want)
        return want

    def check(self, i, got):
        step = self.sched.steps[i]
        try:
            check(step, got, self.want(i))
        except Mismatch as e:
            before = "".join("\n    step %d: %s" % (j, self.sched.steps[j].describe()) for j in range(max(i - 3, 0), i))
            raise Mismatch("schedule %s, step %d of %d: %s\n  %s\n  the steps before it:%s" % (
                self.sched.name, i, len(self.sched.steps), e, step.describe(), before or " none")) from None


# ---- hand-made schedules ----------------------------------------------------------------------------------------------------

def mask_tail():
    """A text of one-byte chunks (the mask all ones, the chunk ends in a list of their own), every small length, the same again."""
    b = _Builder("mask_tail", mask_tail.__doc__)
    b.add("plain", "ones", offsets=True).add("count", "ones", reset=True)
    for route in ("plain", "byteoff", "count"):
        for k, name in enumerate(SMALL):
            b.add(route, name, text=("host", "dev", "dev1")[k % 3], offsets=route != "count", out="host")
            b.add(route, name, text=("dev", "dev1", "host")[k % 3], offsets=route != "count" and k % 2 == 0,
                  out="dev" if route != "count" else "host", bits=16 if k % 2 else 32)
    b.add("plain", "ones", offsets=True).add("byteoff", "ones", out="dev").add("count", "ones")
    return b.sched


def singles_shrink():
    """300 NUL-led numbers in a device text, then 3, then none; a caller's list of one; an id that 16 bits cannot hold; none again."""
    b = _Builder("singles_shrink", singles_shrink.__doc__)
    b.add("plain", "large", text="dev", offsets=True).add("byteoff", "large", text="dev", offsets=True)
    b.add("plain", "medium", text="dev", offsets=True).add("byteoff", "medium", text="dev1", out="dev")
    b.add("plain", "s65", text="dev", offsets=True).add("byteoff", "s1025", text="dev")
    inp = pool()["s1025"]
    off = inp.chunk_off.astype(np.int64)
    c = len(off) // 2
    one = ((int(off[c]), int(off[c + 1] - off[c]), 300),)
    b.add("endmask", "s1025", singles=one).add("endmask", "s1025", singles=one, byteoff=True, out="dev")
    b.add("endmask", "s1025", singles=((one[0][0], one[0][1], 70000),), bits=16)             # MBPE_ERR_VOCAB
    b.add("endmask", "s1025", singles=((one[0][0], one[0][1], 70000),), bits=32)
    b.add("plain", "s1025", text="dev", offsets=True).add("endmask", "s65", singles=()).add("byteoff", "s33", text="dev")
    b.add("endmask", "large", byteoff=True).add("plain", "large", text="dev", offsets=True, bits=16)
    return b.sched


def docs_shrink():
    """1,025 documents and more through the four packers, on the host route and the endmask route; then one document; then no token; then all again."""
    b = _Builder("docs_shrink", docs_shrink.__doc__)
    k = 0
    for name in ("large", "s33", "s0", "large"):
        for endmask in (False, True):
            for route, pack in (("pack", dict(layout="padded", bos=BOS)), ("pack", dict(layout="packed")),
                                ("aux", dict(layout="packed")), ("aux", dict(layout="padded", pad_left=True)),
                                ("windows", {}), ("fit", dict(seq_len=32, bos=BOS))):
                b.add(route, name, endmask=endmask, pack=pack, out=("host", "dev")[k % 2], text=("host", "dev")[k // 2 % 2])
                k += 1
    return b.sched


def stages_toggle():
    """FIM on a large batch, off on a small one; whole-word MLM on a large one, token MLM in 16 bits on a small one; both (refused); FIM alone; neither."""
    b = _Builder("stages_toggle", stages_toggle.__doc__)

    def three(name, **kw):
        for k, route in enumerate(("aux", "windows", "fit")):
            b.add(route, name, endmask=bool(k % 2) ^ (name != "large"), pack=dict(layout="packed"), **kw)
    b.set(fim=FIM_ONE)
    three("large")
    b.set(fim=None)
    three("s1025")
    b.set(mlm=MLM_WORD)
    three("large", out="dev")
    b.add("aux", "medium", bits=16)                                  # whole words in 16 bits: MBPE_ERR_ARG
    b.set(mlm=MLM_TOKEN)
    three("s1023", bits=16)
    b.set(fim=FIM_HALF)
    three("medium")                                                  # both stages: MBPE_ERR_ARG
    b.set(mlm=None)
    three("medium")
    b.add("pack", "medium", pack=dict(layout="packed"))
    b.set(fim=None)
    three("s65")
    three("large")
    return b.sched


def order_and_dropout():
    """Greedy large, rank small, dropout 1 large, dropout 0 small, dropout 0.3 in four pieces, greedy with dropout (refused), greedy, rank large."""
    b = _Builder("order_and_dropout", order_and_dropout.__doc__)
    b.add("plain", "large", offsets=True).add("byteoff", "large")
    b.set(order="rank").add("plain", "s65", offsets=True).add("byteoff", "s33", out="dev")
    b.set(dropout=(1.0, 7)).add("plain", "large", offsets=True).add("byteoff", "large", text="dev")
    b.set(dropout=(0.0, 7)).add("plain", "s1025", offsets=True).add("byteoff", "s64")
    medium = pool()["medium"]
    b.set(dropout=(0.3, 5), piece_bytes=len(medium.data) // 4 + 8)
    b.add("plain", "medium", offsets=True).add("byteoff", "medium").add("count", "medium", reset=True)
    b.add("aux", "medium", pack=dict(layout="packed"))
    b.set(order="greedy", piece_bytes=0).add("plain", "medium").add("count", "medium")            # MBPE_ERR_ARG twice
    b.set(dropout=None).add("plain", "s1023", offsets=True).add("byteoff", "s31").add("count", "s31")
    b.set(order="rank").add("plain", "large", offsets=True).add("byteoff", "large", out="dev").add("count", "large")
    return b.sched


def dedup_toggle():
    """Through the unique chunks: a large text with both limits, off for a small one, on for a small one, the endmask call with singles and documents, counts on both routes."""
    b = _Builder("dedup_toggle", dedup_toggle.__doc__)
    b.set(dedup=True).add("plain", "large", offsets=True).add("plain", "large", out="dev", bits=16, text="dev")
    b.set(dedup_max=0).add("plain", "large", offsets=True).add("pack", "large", pack=dict(layout="packed"))
    b.set(dedup_max=256, dedup=False).add("plain", "s1025", offsets=True).add("aux", "s65")
    b.set(dedup=True).add("plain", "s1023", offsets=True).add("plain", "s0").add("byteoff", "s33")      # (the last: refused)
    b.add("endmask", "large").add("endmask", "medium", out="dev").add("aux", "medium", endmask=True, pack=dict(layout="packed"))
    b.add("windows", "large", endmask=True, out="dev").add("fit", "medium")
    b.add("count", "large", reset=True).add("count", "s65")
    b.set(dedup=False).add("count", "medium", reset=True).add("count", "large")
    b.set(dedup=True).add("count", "medium", endmask=True).add("plain", "large", offsets=True)
    return b.sched


def widths_and_sides():
    """One medium text as 32-bit device, 16-bit host, 16-bit device, 32-bit host output, a query, a cap one too small, 32-bit host again; flat, then packed."""
    b = _Builder("widths_and_sides", widths_and_sides.__doc__)
    forms = (dict(out="dev", bits=32), dict(out="host", bits=16), dict(out="dev", bits=16), dict(out="host", bits=32),
             dict(cap="query"), dict(out="dev", cap="short"), dict(out="host", cap="short"), dict(out="host", bits=32))
    for route, kw in (("plain", dict(offsets=True)), ("pack", dict(pack=dict(layout="packed")))):
        for f in forms:
            if route == "pack" and f == dict(out="host", cap="short"):
                continue                                             # (the binding sizes a host matrix itself)
            b.add(route, "medium", **dict(kw, **f))
    return b.sched


def pieces_flip():
    """piece_bytes 0, a quarter of the text, 0, less than the longest chunk (refused), 0: flat tokens, byte offsets for the host, counts."""
    b = _Builder("pieces_flip", pieces_flip.__doc__)
    large = pool()["large"]
    longest = int(np.diff(large.chunk_off.astype(np.int64)).max())
    first = True
    for piece in (0, len(large.data) // 4, 0, longest - 1, 0):
        b.set(piece_bytes=piece)
        b.add("plain", "large", offsets=True).add("byteoff", "large", offsets=True).add("count", "large", reset=first)
        b.add("plain", "s1025", offsets=True)
        first = False
    return b.sched


HAND_MADE = (mask_tail, singles_shrink, docs_shrink, stages_toggle, order_and_dropout, dedup_toggle, widths_and_sides,
             pieces_flip)


@functools.lru_cache(maxsize=None)
def hand_made(name):
    return {f.__name__: f for f in HAND_MADE}[name]()


# ---- constructed schedules ----------------------------------------------------------------------------------------------------

def euler_circuit(rng, n=len(ROUTES)):
    """An Eulerian circuit of the complete directed graph on n vertices with self-loops (n * n edges), by Hierholzer's
    walk with the seed's choice of the next edge -> the n * n + 1 vertices it passes, the first repeated at the end."""
    left = {v: list(range(n)) for v in range(n)}
    for v in left:
        rng.shuffle(left[v])
    stack, circuit = [rng.randrange(n)], []
    while stack:
        v = stack[-1]
        if left[v]:
            stack.append(left[v].pop())
        else:
            circuit.append(stack.pop())
    circuit.reverse()
    return circuit


SEEDS = (1, 2, 3, 4)
# the settings a constructed schedule toggles: name -> (off, on).  Both values are valid with any other setting or give
# one documented refusal, which refusal() names.
TOGGLES = {
    "order": ("greedy", "rank"), "dropout": (None, (0.25, 3)), "dedup": (False, True), "dedup_max": (256, 0),
    "piece_bytes": (0, 20000), "fim": (None, FIM_HALF), "mlm": (None, MLM_TOKEN), "count_ids": (0, 70001),
}
# the steps [a, b) at which each is on, before the seed moves every edge by up to two steps: on, off, on and off again,
# dropout mostly inside the rank order and outside "dedup", the two stages mostly apart -- a few steps of every
# refused combination, and most steps calls that succeed
ON = {
    "order": ((4, 30), (38, 58)), "dropout": ((10, 18), (42, 50)), "dedup": ((16, 26), (48, 56)),
    "dedup_max": ((20, 34), (52, 60)), "piece_bytes": ((6, 14), (30, 44)), "fim": ((8, 21), (36, 46)),
    "mlm": ((20, 28), (44, 54)),
}
# ("count_ids" reaches the count steps alone and changes only with a reset: it follows their number, two off, two on)


def _phase_sizes(classes):
    """Per step, by construction: the first occurrence of a class is large, its second small, its last large again,
    the occurrences between them large, medium and small in turn."""
    seen, last = {}, {c: max(i for i, x in enumerate(classes) if x == c) for c in set(classes)}
    out = []
    for i, c in enumerate(classes):
        k = seen.get(c, 0)
        seen[c] = k + 1
        if k == 0 or i == last[c]:
            out.append("large")
        elif k == 1:
            out.append("small")
        else:
            out.append(("medium", "small", "large")[k % 3])
    return out


@functools.lru_cache(maxsize=None)
def constructed(seed):
    """64 transitions + 1 steps; the seed picks the circuit, the small inputs, when the settings change, the sides, the
    width and the cap.  Every setting is switched on, off and on again with calls in between (ON)."""
    rng = random.Random(seed)
    classes = [ROUTES[v] for v in euler_circuit(rng)]
    sizes = _phase_sizes(classes)
    b = _Builder("constructed-%d" % seed, "Eulerian circuit of the route classes, seed %d" % seed)
    on = {k: [(a + rng.randrange(-2, 3), b + rng.randrange(-2, 3)) for a, b in ON[k]] for k in sorted(ON)}
    n_count = 0
    for i, (route, size) in enumerate(zip(classes, sizes)):
        cur = {k: TOGGLES[k][int(any(a <= i < b for a, b in on[k]))] for k in sorted(ON)}
        cur["count_ids"] = TOGGLES["count_ids"][n_count // 2 % 2]
        n_count += route == "count"
        # count_ids may change only while the table is empty: the step resets it first
        reset = route == "count" and (cur["count_ids"] != b.cur["count_ids"] or rng.random() < 0.3)
        if route != "count":
            cur["count_ids"] = b.cur["count_ids"]                     # (it takes effect at the next count step)
        b.set(**cur)
        inp = size if size != "small" else SMALL[rng.randrange(len(SMALL))]
        bits = rng.choice((16, 32))
        out = rng.choice(("host", "dev"))
        text = rng.choice(("host", "dev", "dev1"))
        cap = rng.choice(("n", "n", "n", "query", "short"))
        if inp == "s0" and cap == "short":
            cap = "n"                                                 # (no count is one below zero)
        endmask = route == "endmask" or (route != "plain" and route != "byteoff" and rng.random() < 0.4)
        kw = dict(text=text, out=out, bits=bits, cap=cap, endmask=endmask)
        if route in BATCH:
            if cap == "short" and out == "host":
                kw["out"] = "dev"                                     # (the binding sizes a host matrix itself)
            layout = rng.choice(("padded", "packed"))
            kw["pack"] = dict(layout=layout, seq_len=rng.choice((9, 24, 33)), bos=rng.choice((None, BOS)),
                              eos=rng.choice((None, EOS)), stride=rng.choice((0, 3)), score_once=rng.random() < 0.5,
                              pad_left=layout == "padded" and rng.random() < 0.3,
                              trunc_left=layout == "padded" and rng.random() < 0.3)
            if route in ("windows", "fit"):
                kw["pack"].update(layout="padded" if route == "windows" else "packed", pad_left=False, trunc_left=False)
        elif route == "count":
            kw = dict(text=text, endmask=endmask, reset=reset)
        else:
            kw.update(offsets=rng.random() < 0.6, docs=rng.random() < 0.7, byteoff=route == "byteoff" or
                      (route == "endmask" and rng.random() < 0.4))
            if route == "endmask" and inp in SMALL and rng.random() < 0.5:
                kw["singles"] = ()
        b.add(route, inp, **kw)
    return b.sched


def all_schedules():
    return [hand_made(f.__name__) for f in HAND_MADE] + [constructed(s) for s in SEEDS]


# ---- a stand-in encoder with one stale-state defect -----------------------------------------------------------------------

DEFECTS = ("stale_mask", "stale_singles", "stale_docs", "stale_stage", "wide_store")


class StandIn:
    """Answers every step from expected(step), as a correct encoder would -- except for ONE defect of the kind this
    suite exists to catch: state of an earlier call that leaks into a later one.  The model of each defect is written at
    the level of the buffer it lives in; tests/test_history_cases_cpu.py predicts, from the schedule alone, the first
    step at which check() must fail.
      stale_mask     the chunk-end mask is written up to the call's length and never cleared behind it, and the kernel
                     that counts the ends reads whole 32-bit words: ends of an earlier, longer call in the last word
                     are counted
      stale_singles  the list of one-token ranges is appended to, never cleared: a range of an earlier call that lies
                     inside the new text is patched into the new tokens
      stale_docs     the document offsets are written for the new n_docs, the rows are made for the most documents any
                     call had
      stale_stage    a stage that was on stays on when the setting is taken back
      wide_store     16-bit ids are written with 32-bit stores"""

    def __init__(self, defect):
        assert defect is None or defect in DEFECTS
        self.defect = defect
        self.mask = np.zeros(0, dtype=bool)          # end bits as the device buffer holds them
        self.singles = []
        self.most_docs = 0
        self.stage = dict(fim=None, mlm=None)
        self.counts = CountTable()

    def run(self, step):
        inp = pool()[step.inp]
        want = expected(step)
        got = copy.deepcopy({k: v for k, v in want.items() if k != "delta"})
        ok = want["error"] == OK
        n = len(inp.data)
        if step.out == "dev" and ok:
            got["guards"] = {}
        if step.route == "count":
            got["counts"] = self.counts.add(step, want)
        # -- stale_mask
        ends = np.zeros(n, dtype=bool)
        ends[inp.chunk_off[1:][np.diff(inp.chunk_off.astype(np.int64)) > 0].astype(np.int64) - 1] = True
        words = -(-n // 32) * 32
        if self.defect == "stale_mask" and ok:
            stale = int(self.mask[n:words].sum()) if len(self.mask) > n else 0
            if stale:
                for key in ("n_out", "n_tokens"):
                    if key in got:
                        got[key] += stale
        if len(self.mask) < words:
            self.mask = np.concatenate([self.mask, np.zeros(words - len(self.mask), dtype=bool)])
        self.mask[:n] = ends                                          # (nothing is cleared behind n)
        # -- stale_singles
        mine = list(_singles_key(step)) if step.endmask else list(nul_singles(step.inp))
        if self.defect == "stale_singles" and ok:
            stale = [r for r in self.singles if r[0] + r[1] <= n and r not in mine]
            if stale:
                for key in ("n_out", "n_tokens"):
                    if key in got:
                        got[key] += len(stale)
        self.singles += [r for r in mine if r not in self.singles]
        # -- stale_docs
        if self.defect == "stale_docs" and ok and step.route in BATCH and self.most_docs > inp.n_docs:
            got["n_rows"] += self.most_docs - inp.n_docs
        if step.route in BATCH:
            self.most_docs = max(self.most_docs, inp.n_docs)
        # -- stale_stage
        if self.defect == "stale_stage" and step.route in BATCH:
            kept = {k: (step.set[k] if step.set[k] is not None else self.stage[k]) for k in ("fim", "mlm")}
            if kept != {k: step.set[k] for k in kept}:
                other = expected(dataclasses.replace(step, set=dict(step.set, **kept)))
                got = copy.deepcopy(other)
                if step.out == "dev" and other["error"] == OK:
                    got["guards"] = {}
        for k in ("fim", "mlm"):
            if step.set[k] is not None:
                self.stage[k] = step.set[k]
        # -- wide_store
        if self.defect == "wide_store" and ok and step.bits == 16 and step.cap != "query":
            for key in ("tokens", "ids"):
                if key in got:
                    a = got[key]
                    buf = np.full(a.size + GUARD, SENTINEL[2], dtype=np.uint16)
                    wide = a.reshape(-1).astype(np.uint32).view(np.uint16)[:len(buf)]
                    buf[:len(wide)] = wide
                    got[key] = buf[:a.size].reshape(a.shape)
                    if step.out == "dev":
                        got["guards"][key] = buf[a.size:]
        return got


# ---- one Tokenizer, 24 calls ------------------------------------------------------------------------------------------------

# the gpt4 split pattern for ASCII text: \p{L} and \p{N} are the ASCII letters and digits there, and the possessive
# quantifiers of the original change nothing (what they would refuse to give back could not help the rest to match)
GPT4_ASCII = re.compile(rb"'(?i:[sdmt]|ll|ve|re)|[^\r\nA-Za-z0-9]?[A-Za-z]+|[0-9]{1,3}| ?[^\sA-Za-z0-9]+[\r\n]*|\s*[\r\n]|\s+(?!\S)|\s+")


def gpt4_chunks(part):
    """-> the ends of the pattern's matches in an ASCII text, which they tile"""
    assert max(part, default=0) < 128
    ends, at = [], 0
    for m in GPT4_ASCII.finditer(part):
        assert m.start() == at and m.end() > at
        at = m.end()
        ends.append(at)
    assert at == len(part)
    return ends


@functools.lru_cache(maxsize=None)
def tokenizer_specials():
    return B.parse_special(read_data("special1.txt"))


@functools.lru_cache(maxsize=None)
def tokenizer_texts():
    """name -> list of texts (documents): medium and small, ASCII, with special tokens of special1.txt inside, at the
    start and at the end, an empty text among them."""
    ts = bytes(c for c in read_data("taylorswift.txt")[60000:80000] if c < 128 and c != 0)
    medium = [ts[:700] + b"<|endoftext|>" + ts[700:900], b"", ts[900:1500], b"<|fim_prefix|>" + ts[1500:1530],
              ts[1530:2400] + b"<|endofprompt|>", ts[2400:2401], b"<|endoftext|><|endoftext|>", ts[2500:3000]]
    small = [ts[4000:4033], b"<|endoftext|>", ts[4100:4165]]
    return {"medium": medium, "small": small, "one": [ts[5000:5065] + b"<|fim_suffix|>" + ts[5065:5100]]}


def tokenizer_buffer(texts, device_split):
    """The buffer a route hands the encoder for these texts laid end to end -> (buffer, chunk_off, singles, the chunk
    index every document starts at).  Host split: the pattern's matches of the parts between special tokens, a special
    token as the chunk NUL + decimal id (singles "nul").  Device split: the text as it is, the occurrences of the
    special tokens as singles."""
    special = tokenizer_specials()
    buf, off, singles, doc_chunk = b"", [0], [], [0]
    for text in texts:
        for a, b, sid in (B.split_special(text, special) if text else []):
            if sid is None:
                off += [len(buf) + e for e in gpt4_chunks(text[a:b])]
                buf += text[a:b]
            else:
                piece = text[a:b] if device_split else b"\0%d" % sid
                singles.append((len(buf), len(piece), sid))
                buf += piece
                off.append(len(buf))
        doc_chunk.append(len(off) - 1)
    return buf, np.array(off, dtype=np.uint64), (tuple(singles) if device_split else "nul"), np.array(doc_chunk, dtype=np.int64)


TOK_FIM = F.spec(rate=F.ONE // 2 + F.ONE // 4, spm=F.ONE // 2, seed=6, doc_base=10, pre=100258, suf=100260, mid=100259)
TOK_MLM = M.spec(M.threshold(0.4), seed=31, doc_base=1000, mask_id=100259, vocab_n=500, whole_word=1, protect=(100257,))
TOK_PACK = dict(seq_len=48, pad_id=0, bos_id=100258, eos_id=100257)


def tokenizer_calls():
    """24 calls for ONE Tokenizer -> (method, texts name, keywords).  Every option of order=, dropout=, dedup=, fim=, mlm=
    and device_split= is present, absent and present again over the list, and an option a call does not name must be
    off for it."""
    aux = dict(labels=True, positions=True, segments=True)
    rank, drop = dict(order="rank"), dict(order="rank", dropout=0.3, seed=5)
    return [
        ("encode", "medium", dict(device_split=True)),
        ("encode", "small", {}),
        ("encode_batch", "medium", dict(device_split=True, **rank)),
        ("encode_batch", "small", dict(**drop)),
        ("encode_batch_padded", "medium", dict(layout="padded")),
        ("encode_batch_padded", "small", dict(layout="packed", dedup=True, **rank)),
        ("encode_batch_aux", "medium", dict(layout="packed", fim=TOK_FIM, **aux)),
        ("encode_batch_aux", "small", dict(layout="packed", **aux)),
        ("encode_batch_aux", "medium", dict(layout="padded", mlm=TOK_MLM, dedup=True, **aux)),
        ("encode_batch_windows", "one", dict(stride=8, score_once=True, row_doc=True, row_tok0=True, **aux)),
        ("encode_batch_windows", "medium", dict(stride=8, score_once=True, row_doc=True, row_tok0=True, fim=TOK_FIM,
                                                device_split=True, **drop, **aux)),
        ("encode_batch_fit", "small", dict(doc_row=True, doc_col=True, **aux)),
        ("encode_batch_fit", "medium", dict(doc_row=True, doc_col=True, mlm=TOK_MLM, **rank, **aux)),
        ("token_counts", "medium", {}),
        ("token_counts", "small", dict(device_split=True, dedup=True)),
        ("encode", "medium", dict(**drop)),
        ("encode", "one", dict(dedup=True)),
        ("encode_batch", "medium", {}),
        ("encode_batch_aux", "small", dict(layout="packed", mlm=TOK_MLM, device_split=True, **aux)),
        ("encode_batch_padded", "medium", dict(layout="packed", fim=TOK_FIM)),
        ("encode_batch_fit", "medium", dict(doc_row=True, doc_col=True, **aux)),
        ("encode_batch_windows", "small", dict(stride=8, score_once=False, row_doc=True, row_tok0=True, mlm=TOK_MLM, **rank,
                                               **aux)),
        ("token_counts", "medium", dict(**drop)),
        ("encode", "small", dict(device_split=True, **rank)),
    ]


def tokenizer_expected(method, name, kw):
    """What a call of tokenizer_calls() must give, from the call alone."""
    texts = tokenizer_texts()[name]
    if method == "encode":
        texts = [b"".join(texts)]
    split = bool(kw.get("device_split"))
    buf, off, singles, doc_chunk = tokenizer_buffer(texts, split)
    order = kw.get("order", "greedy")
    dropout = (kw["dropout"], kw["seed"]) if kw.get("dropout") else None
    tok, ends, _ = stream_of_text(buf, off, order, dropout, singles)
    doc_tok = R.chunk_tok_off(ends, len(buf), off)[doc_chunk].astype(np.uint64)
    if method == "encode":
        return tok
    if method == "encode_batch":
        return [tok[int(a):int(b)] for a, b in zip(doc_tok[:-1], doc_tok[1:])]
    if method == "token_counts":
        return H.reference(tok, max(n_table_ids(), max(tokenizer_specials().values()) + 1))[0]
    route = {"encode_batch_padded": "pack", "encode_batch_aux": "aux", "encode_batch_windows": "windows",
             "encode_batch_fit": "fit"}[method]
    pack = dict(seq_len=TOK_PACK["seq_len"], pad=TOK_PACK["pad_id"], bos=TOK_PACK["bos_id"], eos=TOK_PACK["eos_id"])
    pack.update({k: kw[k] for k in ("layout", "stride", "score_once") if k in kw})
    step = Step(route, "s0", dict(DEFAULTS, fim=kw.get("fim"), mlm=kw.get("mlm")), pack=pack)
    want = matrices(step, tok, ends, doc_tok)
    return {k: v for k, v in want.items() if k not in ("error", "n_rows", "n_tokens", "fim_info", "cu_seqlens", "max_seqlen")}
