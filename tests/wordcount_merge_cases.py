"""Merging word-count tables, restated in Python on top of tests/wordcount_cases.py: the reference of
tests/test_wordcount_merge_cpu.py and of the GPU tests (test_gpu_wordcount_merge.py, test_gpu_train_counts_tokenizer.py).
Accumulator.merge is the rule of the merge on lists -- it never calls add -- and blob() writes the serialised table of
csrc/wordcount.h field by field, so that a test can write one that breaks a single rule."""
import struct

import dedup_cases as C
import wordcount_cases as W

MAGIC = 0x4357424D                  # "MBWC"
VERSION = 1
HEADER = 64


class Accumulator(W.Accumulator):
    """W.Accumulator with the merge of another table.  Its lists hold no empty chunks, so the chunks of the concatenated
    list before the next piece (chunk_base) are n_chunks_total."""

    @property
    def chunk_base(self):
        return self.n_chunks_total

    def merge(self, other):
        """Per entry of `other`, in its order: found here -> the weight is added; not found -> appended with first_chunk =
        this table's chunk_base + its first_chunk; above max_chunk_bytes -> appended without a look.  Then the totals grow
        by the other's."""
        assert other is not self and other.max_chunk_bytes == self.max_chunk_bytes
        base = self.chunk_base
        for c, wc, fc in zip(other.uniq, other.weights, other.first):
            hashed = len(c) <= self.max_chunk_bytes
            j = self.index.get(c) if hashed else None
            if j is not None:
                self.weights[j] += wc
                continue
            if hashed:
                self.index[c] = len(self.uniq)
            self.uniq.append(c)
            self.weights.append(wc)
            self.first.append(base + fc)
        self.n_chunks_total += other.n_chunks_total
        self.n_pieces += other.n_pieces


def count(pieces, max_chunk_bytes=C.MAX_CHUNK_BYTES, repeats=None):
    """One table counted from the pieces, by add alone."""
    acc = Accumulator(max_chunk_bytes)
    for k, p in enumerate(pieces):
        acc.add(p, 1 if repeats is None else repeats[k])
    return acc


def table(acc):
    """What the tests compare: everything the statement covers."""
    return acc.uniq, acc.weights, acc.first, acc.n_chunks_total, acc.n_pieces


def groups(pieces, n_tables):
    """The pieces in n_tables consecutive groups, as W.cut_list cuts chunks."""
    return W.cut_list(pieces, n_tables)


def blob(uniq, weights, first, n_pieces, n_chunks_total, chunk_base, max_chunk_bytes=C.MAX_CHUNK_BYTES, magic=MAGIC,
         version=VERSION, ends=None, n_unique=None, n_bytes=None):
    """The serialised table, little-endian: a 64-byte header (u32 magic, u32 version, u64 max_chunk_bytes, n_unique,
    n_bytes, n_pieces, n_chunks_total, chunk_base, 0), then ends, weights and first_chunk as u64, then the text padded
    with zeros to 16 bytes.  ends, n_unique and n_bytes default to what uniq gives; a test overrides one to break it."""
    text = b"".join(uniq)
    if ends is None:
        ends, at = [], 0
        for c in uniq:
            at += len(c)
            ends.append(at)
    head = struct.pack("<II7Q", magic, version, max_chunk_bytes, len(uniq) if n_unique is None else n_unique,
                       len(text) if n_bytes is None else n_bytes, n_pieces, n_chunks_total, chunk_base, 0)
    assert len(head) == HEADER
    arrays = b"".join(struct.pack("<%dQ" % len(v), *v) for v in (ends, weights, first))
    return head + arrays + text + b"\0" * (-len(text) % 16)


def blob_of(acc, **kw):
    return blob(acc.uniq, acc.weights, acc.first, acc.n_pieces, acc.n_chunks_total, acc.chunk_base,
                kw.pop("max_chunk_bytes", acc.max_chunk_bytes), **kw)


def corrupt_blobs(acc):
    """name -> a blob of acc's table with one field edited so that exactly one rule of the check is broken.  acc needs
    at least three hashed entries."""
    u, w, f = list(acc.uniq), list(acc.weights), list(acc.first)
    good = blob_of(acc)
    ends, at = [], 0
    for c in u:
        at += len(c)
        ends.append(at)
    swapped = list(ends)
    swapped[1] = swapped[0]
    zero = list(w)
    zero[1] = 0
    first = list(f)
    first[2] = first[1]
    twice = list(u)
    twice[2] = twice[0]             # (the ends follow the bytes: every other rule still holds)
    return {
        "truncated": good[:-16],
        "bad magic": blob_of(acc, magic=MAGIC ^ 1),
        "other max_chunk_bytes": blob_of(acc, max_chunk_bytes=acc.max_chunk_bytes - 1),
        "an end out of order": blob_of(acc, ends=swapped),
        "weight 0": blob(u, zero, f, acc.n_pieces, acc.n_chunks_total, acc.chunk_base, acc.max_chunk_bytes),
        "first_chunk out of order": blob(u, w, first, acc.n_pieces, acc.n_chunks_total, acc.chunk_base,
                                         acc.max_chunk_bytes),
        "weights' sum": blob(u, w, f, acc.n_pieces, acc.n_chunks_total + 1, acc.chunk_base + 1, acc.max_chunk_bytes),
        "a hashed chunk twice": blob(twice, w, f, acc.n_pieces, acc.n_chunks_total, acc.chunk_base, acc.max_chunk_bytes),
    }
