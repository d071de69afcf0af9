"""The masked-LM rule (include/mbpe.h, mbpe_mlm_spec) restated in Python: what mbpe_mlm_plan, mbpe_mlm_tokens and the
encoder's stage are held to, the labels the packers make of a target stream, and the case lists of the CPU and GPU
tests."""
import random

import numpy as np

from fim_cases import ref_hash

M64 = (1 << 64) - 1
ONE = 1 << 32                       # the threshold of probability 1
NO_TOKEN = 0xFFFFFFFF
END = 1 << 31                       # bit 31 of a 32-bit token: last token of its word
MASK_ID = 50001
VOCAB_N = 50000


def threshold(p):
    return int(p * 4294967296.0)


def spec(select=threshold(0.15), mask=threshold(0.8), random=threshold(0.1), seed=0, doc_base=0, mask_id=MASK_ID,
         vocab_n=VOCAB_N, whole_word=0, protect=()):
    """The rule's parameters as a dict; select, mask and random are thresholds in [0, 2^32]."""
    return dict(select=select, mask=mask, random=random, seed=seed, doc_base=doc_base, mask_id=mask_id, vocab_n=vocab_n,
                whole_word=whole_word, protect=tuple(protect))


def doc_seed(s, d):
    g = (s["doc_base"] + d) & M64
    return (ref_hash(s["seed"], g, 0x4D4C4D00) << 32) | ref_hash(s["seed"], g, 0x4D4C4D01)


def ref_doc(s, d, ids, ends):
    """Document d of the call: ids (plain) and ends (truthy: last token of its word) -> (new ids, targets)."""
    sg = doc_seed(s, d)
    out, tgt, w = [], [], 0
    for k, t in enumerate(ids):
        if k == 0 or not s["whole_word"] or ends[k - 1]:
            w = k
        if ref_hash(sg, w, 0) < s["select"] and t not in s["protect"]:
            tgt.append(t)
            r = ref_hash(sg, k, 1)
            if r < s["mask"]:
                out.append(s["mask_id"])
            elif r < s["mask"] + s["random"]:
                out.append((ref_hash(sg, k, 2) * s["vocab_n"]) >> 32)
            else:
                out.append(t)
        else:
            tgt.append(NO_TOKEN)
            out.append(t)
    return out, tgt


def ref_apply(s, ids, ends, off):
    """A flat stream: ids, ends (one per token) and offsets [n_docs + 1] -> (new ids, targets) as lists."""
    out, tgt = [], []
    for d in range(len(off) - 1):
        a, b = int(off[d]), int(off[d + 1])
        o, t = ref_doc(s, d, ids[a:b], ends[a:b])
        out += o
        tgt += t
    return out, tgt


def stream(lens, rng, word=3.0, hi=VOCAB_N, flag_last=True):
    """Random ids and word ends for documents of these lengths: a token ends its word with probability 1 / word;
    flag_last: a document's last token is flagged as the encoder flags it (the rule does not need it)."""
    ids, ends = [], []
    for L in lens:
        for k in range(L):
            ids.append(rng.randrange(0, hi))
            ends.append(rng.random() * word < 1.0 or (flag_last and k == L - 1))
    off = np.zeros(len(lens) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens, dtype=np.uint64) if len(lens) else []
    return ids, ends, off


def flagged(ids, ends):
    """uint32 tokens with the ends in bit 31"""
    return (np.array(ids, dtype=np.uint32) | (np.array(ends, dtype=bool).astype(np.uint32) << np.uint32(31))) \
        if len(ids) else np.zeros(0, dtype=np.uint32)


def split_lens(n_tokens, rng, n_docs):
    """n_docs document lengths (some 0) that sum to n_tokens"""
    cuts = sorted(rng.randrange(0, n_tokens + 1) for _ in range(n_docs - 1))
    return [b - a for a, b in zip([0] + cuts, cuts + [n_tokens])]


def gpu_cases():
    """(name, ids, ends, off) of the GPU test: the smallest shapes that can break the kernels (1,024 tokens a span, 4
    tokens a 16-byte piece of 32-bit tokens, 8 of 16-bit ones)."""
    rng = random.Random(29)
    cases = []
    for n in (1, 1023, 1024, 1025, 2049):
        cases.append(("n%d" % n,) + stream(split_lens(n, rng, 1 + n // 100), rng))
    cases.append(("tiny",) + stream([0, 1, 2, 0, 5], rng))
    lens = [0] * 1100                                            # about 1,100 documents, most of them empty
    for i in rng.sample(range(1100), 60):
        lens[i] = rng.randrange(1, 70)
    cases.append(("empties",) + stream(lens, rng))
    # a single word of 2,500 tokens between two short documents: span 1 has no start and the carry crosses it
    ids, ends, off = stream([3, 2500, 6], rng)
    for i in range(3, 3 + 2500):
        ends[i] = i == 3 + 2499
    cases.append(("long_word", ids, ends, off))
    # word starts on the first and on the last token of a span, nowhere else near them
    ids, ends, off = stream([3000], rng, word=6.0)
    for i in range(1000, 1050):
        ends[i] = i in (1022, 1023)                              # starts at 1023 (last of span 0) and 1024 (first of span 1)
    for i in range(2030, 2060):
        ends[i] = i in (2046, 2047)
    cases.append(("span_edges", ids, ends, off))
    # document boundaries inside a 16-byte piece, the last token of most documents NOT flagged
    ids, ends, off = stream([1, 1, 3, 2, 5, 6, 7, 1, 9, 1030, 2, 1], rng, flag_last=False)
    cases.append(("unflagged_ends", ids, ends, off))
    return cases


# ---- labels from a target stream: the packers' cells ----------------------------------------------------------------------

def ref_labels(out, tgt, off, nb, ne, ignore, tok0_of_cell):
    """What the packers write as labels with label_tokens, cell by cell, from a call's OTHER outputs: out["segments"]
    (d + 1, 0 = pad) and tok0_of_cell(row, col, d, pos) -> the index in document d of the cell's token, or None where
    the cell holds bos or eos.  A body cell gets its token's target, ignore where that is NO_TOKEN; all others ignore."""
    seg, pos = out["segments"], out["positions"]
    lab = np.full(seg.shape, ignore, dtype=np.int64)
    for r in range(seg.shape[0]):
        for c in range(seg.shape[1]):
            if seg[r, c] == 0:
                continue
            d = int(seg[r, c]) - 1
            k = tok0_of_cell(r, c, d, int(pos[r, c]))
            if k is None:
                continue
            t = tgt[int(off[d]) + k]
            if t != NO_TOKEN:
                lab[r, c] = t
    return lab
