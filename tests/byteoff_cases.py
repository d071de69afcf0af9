"""A position-carrying BPE, the reference of the token byte offset tests (test_byteoff_cpu.py, test_gpu_byteoff.py,
test_gpu_byteoff_tokenizer.py).  Every token is a triple [id, start, end]; a merge of two neighbours keeps the first
one's start and the second one's end.  Nothing here looks at a vocabulary: where a token came from is carried, not
derived from its id -- which is what the product does the other way round (len[id], prefix sums).

Both orders of encode are restated: the reference's greedy passes (any pair in the lookup, first match wins, until a
pass replaces nothing) and rank order (the smallest candidate id of the chunk, every occurrence left to right).  The
split into chunks is not under test and comes from the product's host splitter (mbpe.presplit_ranges)."""
import re

import numpy as np

_STOI = re.compile(rb"[ \t\n\v\f\r]*([+-]?[0-9]+)")


def parse_model(raw):
    lines = raw.decode().split("\n")
    assert lines[0] == "minbpe v1"
    n_special = int(lines[2])
    merges = [tuple(int(v) for v in ln.split()) for ln in lines[3 + n_special:] if ln]
    return lines[1], merges


def parse_special(raw):
    special = {}
    for ln in raw.decode().split("\n"):
        if ln.strip():
            name, idx = ln.rsplit(" ", 1)
            special[name.encode()] = int(idx)
    return special


def vocab_bytes(merges):
    vocab = [bytes([i]) for i in range(256)]
    for a, b in merges:
        vocab.append(vocab[a] + vocab[b])
    return vocab


def stoi_single(chunk):
    """The id a NUL-led chunk collapses to (text_to_vector, Tokenizer.h:86-93), or None."""
    chunk = bytes(chunk)
    if chunk[:1] == b"\0":
        m = _STOI.match(chunk[1:].split(b"\0")[0])
        if m and -(1 << 31) <= int(m.group(1)) < (1 << 31):
            return int(m.group(1)) & 0xFFFFFFFF
    return None


def encode_chunk(chunk, start, lookup, rank=False):
    """chunk: bytes that begin at `start` -> list of [id, start, end]."""
    if not len(chunk):
        return []
    sid = stoi_single(chunk)
    if sid is not None:
        return [[sid, start, start + len(chunk)]]
    toks = [[b, start + i, start + i + 1] for i, b in enumerate(bytes(chunk))]
    while True:
        best = None
        if rank:
            cands = [lookup[(toks[i][0], toks[i + 1][0])] for i in range(len(toks) - 1)
                     if (toks[i][0], toks[i + 1][0]) in lookup]
            if not cands:
                return toks
            best = min(cands)
        out, i, merged = [], 0, False
        while i < len(toks):
            m = lookup.get((toks[i][0], toks[i + 1][0])) if i + 1 < len(toks) else None
            if m is not None and (best is None or m == best):
                out.append([m, toks[i][1], toks[i + 1][2]])
                i += 2
                merged = True
            else:
                out.append(toks[i])
                i += 1
        toks = out
        if not merged:
            return toks


def encode_chunks(data, chunk_off, merges, rank=False):
    """The encoder level: (tokens uint32, tok_byte_off uint64 of n + 1 entries) for the chunks chunk_off of data."""
    data = bytes(data)
    lookup = {tuple(m): 256 + k for k, m in enumerate(merges)}
    off = [0, len(data)] if chunk_off is None else [int(v) for v in chunk_off]
    toks = []
    for s, e in zip(off[:-1], off[1:]):
        toks.extend(encode_chunk(data[s:e], s, lookup, rank))
    for (_, _, e), (_, s, _) in zip(toks[:-1], toks[1:]):
        assert e == s                                     # the chunks tile the text, so the tokens do
    ids = np.array([t[0] for t in toks], dtype=np.uint32)
    boff = np.array([t[1] for t in toks] + [len(data)], dtype=np.uint64)
    return ids, boff


def split_special(text, special):
    """split_on_special (Tokenizer.h:605-650): the earliest occurrence of any name (ties: the first name), cut,
    continue behind it -> list of (start, end, id or None)."""
    parts, pos = [], 0
    while True:
        nxt = None
        for name in special:
            at = text.find(name, pos) if name else -1
            if at >= 0 and (nxt is None or at < nxt[0]):
                nxt = (at, name)
        if nxt is None:
            if pos < len(text) or not parts:
                parts.append((pos, len(text), None))
            return parts
        if nxt[0] > pos:
            parts.append((pos, nxt[0], None))
        pos = nxt[0] + len(nxt[1])
        parts.append((nxt[0], pos, special[nxt[1]]))


def tokenizer_encode(text, pattern, special, merges, rank=False):
    """The Tokenizer level: (tokens uint32, ranges uint64 [n, 2]) in the coordinates of the original text."""
    import mbpe
    text = bytes(text)
    lookup = {tuple(m): 256 + k for k, m in enumerate(merges)}
    toks = []
    for s, e, sid in split_special(text, special):
        if sid is not None:
            toks.append([sid, s, e])
            continue
        part = text[s:e]
        if pattern and part[:1] != b"\0":
            starts, ends = mbpe.presplit_ranges(pattern, part)
            spans = [(s + int(a), s + int(b)) for a, b in zip(starts, ends)]
        else:
            spans = [(s, e)]
        for a, b in spans:
            toks.extend(encode_chunk(text[a:b], a, lookup, rank))
    ids = np.array([t[0] for t in toks], dtype=np.uint32)
    ranges = np.array([t[1:] for t in toks], dtype=np.uint64).reshape(-1, 2)
    return ids, ranges
