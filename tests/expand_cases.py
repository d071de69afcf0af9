"""The shapes of the expansion tests (csrc/expand.h): chunk lists whose token counts are known exactly under a table whose
one merge never applies -- a chunk's token count is then its byte count -- and the naive expansion they are checked
against.  tests/expand_check.cpp generates the same shapes for the host restatement; tests/test_gpu_encode_dedup.py runs
these through the encoder's "dedup" route."""
import numpy as np

SPAN = 1024                      # chunks one wave walks (kExpSpan)

# a table whose only merge never applies to the bytes the generators below use (97 .. 122, 0, digits, spaces)
NEVER = np.array([[1, 2]], dtype=np.uint32)


def expand(runs, unique_of):
    """The tokens of every chunk, one after the other: chunk c copies runs[unique_of[c]] -> (list, chunk ends)."""
    out, ends = [], []
    for j in unique_of:
        out += list(runs[j])
        ends.append(len(out))
    return out, ends


def _word(i, length):
    """A chunk of `length` bytes over a .. z that spells i in base 26 (distinct for distinct i below 26^length)."""
    s = bytearray()
    for _ in range(length):
        s.append(97 + i % 26)
        i //= 26
    return bytes(s)


def equal_chunks(n=700):
    return [b"ab"] * n


def distinct_chunks(n=600):
    return [_word(i, 3) for i in range(n)]


def edge_chunks(n, seed=0):
    """n chunks drawn from a few words of 1 .. 5 bytes: n = 1,023 .. 1,025 and 4,095 .. 4,097 cross the span edge and the
    edge of a two-span workgroup."""
    rng = np.random.default_rng(seed + n)
    pool = [b"a", b"bc", b"def", b"ghij", b"klmno", b"p", b"qq"]
    return [pool[int(k)] for k in rng.integers(0, len(pool), size=n)]


def residue_chunks(r):
    """The first span's 1,024 chunks hold 1,024 + r tokens, so the second span's output starts r elements behind a
    16-byte boundary of an aligned output: r = 0 .. 7 gives every residue for 4-byte and for 2-byte elements."""
    first = [b"a"] * SPAN
    first[17] = b"b" * (1 + r)
    return first + [b"c", b"de"] * 150


def long_chunks(n_long=5000):
    """A chunk of n_long bytes three times between one-byte chunks."""
    big = bytes(97 + (i * 7 + i // 26) % 26 for i in range(n_long))
    return [b"a", big, b"b", big, b"a", b"a", big, b"b"]


def with_empty_chunks(chunks, every=3):
    """(text, chunk_off) of chunks with an empty chunk in front, behind, and after every `every`-th chunk."""
    off = [0, 0]
    for i, c in enumerate(chunks):
        off.append(off[-1] + len(c))
        if i % every == 0:
            off.append(off[-1])
    off.append(off[-1])
    return np.frombuffer(b"".join(chunks), dtype=np.uint8), np.array(off, dtype=np.uint64)


def nul_chunks():
    """NUL-led chunks with a number (one token each) and without (ordinary bytes), repeated, between words."""
    one = [b"ab", b"\x00300", b"cd", b"\x00x1", b"\x00300", b"ab", b"\x00 77", b"\x00", b"\x00x1", b"\x0065000", b"cd"]
    return one * 5
