"""Word counts across pieces, restated in Python on top of tests/dedup_cases.py: the reference of
tests/test_wordcount_cpu.py and of the GPU tests (test_gpu_wordcount.py, test_gpu_train_pieces*.py), and their cuts."""
import dedup_cases as C


class Accumulator:
    """The fold of mbpe_wordcount on lists: every piece is deduplicated on its own (C.dedup) and its result merged into
    the table -- a chunk that is there adds weight x repeat, any other is appended in the piece's order; a chunk above
    max_chunk_bytes is never looked up."""

    def __init__(self, max_chunk_bytes=C.MAX_CHUNK_BYTES):
        self.max_chunk_bytes = max_chunk_bytes
        self.index = {}
        self.uniq, self.weights, self.first = [], [], []
        self.n_pieces = self.n_chunks_total = 0

    def add(self, chunks, repeat=1):
        chunks = [c for c in chunks if c]
        u, w, f = C.dedup(chunks, self.max_chunk_bytes)
        for c, wc, fc in zip(u, w, f):
            j = self.index.get(c) if len(c) <= self.max_chunk_bytes else None
            if j is None:
                if len(c) <= self.max_chunk_bytes:
                    self.index[c] = len(self.uniq)
                self.uniq.append(c)
                self.weights.append(wc * repeat)
                self.first.append(self.n_chunks_total + fc)
            else:
                self.weights[j] += wc * repeat
        self.n_chunks_total += len(chunks) * repeat
        self.n_pieces += 1

    def result(self):
        return self.uniq, self.weights, self.first


def accumulate(pieces, max_chunk_bytes=C.MAX_CHUNK_BYTES):
    acc = Accumulator(max_chunk_bytes)
    for p in pieces:
        acc.add(p)
    return acc.result()


def concat(pieces):
    return [c for p in pieces for c in p if c]


def cut_list(chunks, n_pieces):
    """chunks in n_pieces consecutive pieces of about the same number of chunks."""
    n = len(chunks)
    return [chunks[k * n // n_pieces:(k + 1) * n // n_pieces] for k in range(n_pieces)]


def cut_text(text, n_pieces):
    """text (bytes) in n_pieces pieces, cut where a letter or digit is followed by whitespace -- a chunk boundary under
    gpt2 and gpt4: for cut k the first index i >= k * n / n_pieces with text[i - 1] in [0-9A-Za-z] and text[i] in
    " \\t\\r\\n"."""
    n = len(text)
    at = [0]
    for k in range(1, n_pieces):
        i = max(k * n // n_pieces, at[-1], 1)
        while i < n and not (chr(text[i - 1]).isascii() and chr(text[i - 1]).isalnum() and text[i] in b" \t\r\n"):
            i += 1
        at.append(i)
    at.append(n)
    return [text[at[k]:at[k + 1]] for k in range(n_pieces)]
