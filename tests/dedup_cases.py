"""Chunk deduplication and training on unique chunks with counts, restated in Python: the references of
tests/test_dedup_cpu.py and of the GPU tests (test_gpu_dedup.py, test_gpu_train_weighted.py), and their generators."""
import numpy as np

MAX_CHUNK_BYTES = 256


def chunks_of(data, off):
    """The chunks of data (bytes) under the offsets off, empty ones dropped -> list of bytes."""
    data = bytes(data)
    off = [int(x) for x in off]
    return [data[off[i]:off[i + 1]] for i in range(len(off) - 1) if off[i + 1] > off[i]]


def join(chunks):
    """list of bytes -> (text as uint8 array, uint64 offsets)."""
    off = np.zeros(len(chunks) + 1, dtype=np.uint64)
    if chunks:
        off[1:] = np.cumsum([len(c) for c in chunks], dtype=np.uint64)
    return np.frombuffer(b"".join(chunks), dtype=np.uint8), off


def dedup(chunks, max_chunk_bytes=MAX_CHUNK_BYTES):
    """The distinct chunks in order of first occurrence -> (unique chunks, weights, first_chunk).  A chunk longer than
    max_chunk_bytes is never merged with its duplicates: it appears with weight 1 as often as it occurs."""
    index = {}
    uniq, weights, first = [], [], []
    for i, c in enumerate(chunks):
        j = index.get(c) if len(c) <= max_chunk_bytes else None
        if j is None:
            if len(c) <= max_chunk_bytes:
                index[c] = len(uniq)
            uniq.append(c)
            weights.append(1)
            first.append(i)
        else:
            weights[j] += 1
    return uniq, weights, first


def end_mask(off, n_bytes):
    """The end mask of the device layout (2 * ceil(n / 16) + 16 bytes) for chunk offsets off."""
    mask = np.zeros((n_bytes + 15) // 16 * 2 + 16, dtype=np.uint8)
    for e in np.asarray(off, dtype=np.int64)[1:]:
        if e > 0:
            mask[(e - 1) >> 3] |= np.uint8(1 << ((e - 1) & 7))
    return mask


def weighted_bpe(chunks, weights, vocab_size, first_mode, start=None, with_seqs=False):
    """BPE on chunks with weights -> (merges, counts).
    Lexical: one table, counted once and then updated by every merge as the reference's walk does -- (a, b) - w,
    (x, a) - w, (x, X) + w with x the left neighbour as already rewritten, (b, y) - w, (X, y) + w with y the right
    neighbour as it still is; a pair stays in the table at count 0.  The choice is the largest weighted count, then the
    smallest (first, second), until the vocabulary is full.
    first: the table is recounted before every merge; among the pairs of maximal weighted count the one whose first
    occurrence in the stream of chunks is earliest wins; the loop ends when no pair is left.
    start: token sequences that already hold ids 256 .. 255 + n in place of `chunks` as bytes, as (sequences, n) -- the
    training continues from merge n, and the merges and counts returned are the new ones only.
    with_seqs: -> (merges, counts, final token sequences)."""
    seqs, k0 = ([list(c) for c in chunks], 0) if start is None else ([list(s) for s in start[0]], int(start[1]))

    def recount():
        cnt, pos = {}, {}
        p = 0
        for s, w in zip(seqs, weights):
            for i in range(len(s) - 1):
                key = (s[i], s[i + 1])
                cnt[key] = cnt.get(key, 0) + w
                pos.setdefault(key, p + i)
            p += len(s)
        return cnt, pos

    tab, _ = recount()
    merges, counts = [], []
    for k in range(k0, vocab_size - 256):
        if first_mode:
            tab, pos = recount()
            if not tab:
                break
            top = max(tab.values())
            a, b = min((pos[key], key) for key, c in tab.items() if c == top)[1]
        else:
            if not tab:
                break
            top = max(tab.values())
            a, b = min(key for key, c in tab.items() if c == top)
        merges.append((a, b))
        counts.append(top)
        X = 256 + k
        for n, (s, w) in enumerate(zip(seqs, weights)):
            if a not in s:
                continue
            out, i = [], 0
            while i < len(s):
                if i + 1 < len(s) and s[i] == a and s[i + 1] == b:
                    tab[(a, b)] = tab.get((a, b), 0) - w
                    if out:
                        x = out[-1]
                        tab[(x, a)] = tab.get((x, a), 0) - w
                        tab[(x, X)] = tab.get((x, X), 0) + w
                    if i + 2 < len(s):
                        y = s[i + 2]
                        tab[(b, y)] = tab.get((b, y), 0) - w
                        tab[(X, y)] = tab.get((X, y), 0) + w
                    out.append(X)
                    i += 2
                else:
                    out.append(s[i])
                    i += 1
            seqs[n] = out
    return (merges, counts, seqs) if with_seqs else (merges, counts)


# ---- generators ------------------------------------------------------------------------------------------------------
def random_chunks(seed, n_chunks, max_len, n_sym, base=97):
    """n_chunks chunks of 1 .. max_len bytes over n_sym symbols."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, max_len + 1, size=n_chunks)
    return [bytes(rng.integers(base, base + n_sym, size=int(n), dtype=np.uint8)) for n in lens]


def distinct_chunks(n_chunks, length=4):
    """n_chunks pairwise distinct chunks of `length` bytes."""
    return [int(i).to_bytes(length, "little") for i in range(1, n_chunks + 1)]


def edge_chunks(seed, total):
    """Chunks of 1 .. 40 bytes, drawn from few values, whose lengths add up to exactly `total` bytes: with total =
    k * 16 - 1, k * 16 and k * 16 + 1 chunk ends fall on and around the 16-byte and the mask-word edges."""
    rng = np.random.default_rng(seed)
    pool = [bytes(rng.integers(97, 100, size=int(n), dtype=np.uint8)) for n in rng.integers(1, 41, size=24)]
    out, left = [], total
    while left > 0:
        c = pool[int(rng.integers(0, len(pool)))][:left]
        out.append(c)
        left -= len(c)
    return out


def long_chunks(max_chunk_bytes=MAX_CHUNK_BYTES):
    """Chunks of max_chunk_bytes - 1, max_chunk_bytes and max_chunk_bytes + 1 bytes, each twice, short ones between."""
    rng = np.random.default_rng(11)
    out = []
    for rep in range(2):
        for n in (max_chunk_bytes - 1, max_chunk_bytes, max_chunk_bytes + 1):
            body = bytes(np.random.default_rng(n).integers(97, 123, size=n, dtype=np.uint8))
            out += [body, bytes(rng.integers(97, 99, size=3, dtype=np.uint8))]
    return out
