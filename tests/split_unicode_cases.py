"""Texts for the tests of the device split's "unicode" mode (test_split_unicode_cpu.py, test_gpu_split_unicode.py):
seeded and generated here, well-formed UTF-8 unless a generator says otherwise."""
import functools

import numpy as np

BLOCK = 64

JOIN = " a\n"


def _scalars(lo, hi):
    return [c for c in range(lo, hi) if not 0xD800 <= c < 0xE000]


@functools.lru_cache(maxsize=None)
def plane_text(plane):
    """Every scalar value c of one plane in the contexts x{c}x, ' {c}{c} ', 1{c}\\n{c}, '{c}l and {c}'s, joined by
    ' a\\n' (a letter in front of whitespace: a sync point between any two of them) -> bytes."""
    parts = []
    for v in _scalars(plane << 16, (plane + 1) << 16):
        c = chr(v)
        parts += ["x" + c + "x", " " + c + c + " ", "1" + c + "\n" + c, "'" + c + "l", c + "'s"]
    return JOIN.join(parts).encode("utf-8")


def every_scalar_value():
    """The 17 plane texts -> (uint8 blob, offsets [18]); joined as they are they also read as one text."""
    texts = [plane_text(p) + (JOIN.encode() if p < 16 else b"") for p in range(17)]
    off = np.zeros(18, dtype=np.uint64)
    np.cumsum([len(t) for t in texts], out=off[1:])
    return np.frombuffer(b"".join(texts), dtype=np.uint8), off


def _pick(rng, pool, n):
    return "".join(pool[i] for i in rng.integers(0, len(pool), n))


def _words(seed, n_bytes, letters, extra=(), lo=1, hi=10):
    rng = np.random.default_rng(seed)
    out, size = [], 0
    seps = [" "] * 12 + [", ", ". ", "\n", " \n", "\n\n", "  ", " - ", "! ", "'s ", " 12 "] + list(extra)
    while size < n_bytes:
        w = _pick(rng, letters, int(rng.integers(lo, hi + 1))) + seps[int(rng.integers(0, len(seps)))]
        out.append(w)
        size += len(w.encode("utf-8"))
    return "".join(out).encode("utf-8")


def cjk(n_bytes=200000, seed=1):
    """Lines of ideographs from U+4E00 - U+9FFF with the two punctuation marks and line feeds; no space anywhere."""
    rng = np.random.default_rng(seed)
    out, size = [], 0
    while size < n_bytes:
        line = ""
        for _ in range(int(rng.integers(1, 6))):
            line += "".join(chr(c) for c in rng.integers(0x4E00, 0xA000, int(rng.integers(1, 14))))
            line += "。，"[int(rng.integers(0, 2))]
        line += "\n" * int(rng.integers(1, 3))
        out.append(line)
        size += len(line.encode("utf-8"))
    return "".join(out).encode("utf-8")


def cyrillic(n_bytes=200000, seed=2):
    return _words(seed, n_bytes, [chr(c) for c in range(0x410, 0x450)])


def greek(n_bytes=50000, seed=3):
    return _words(seed, n_bytes, [chr(c) for c in range(0x391, 0x3CA) if c != 0x3A2])


def devanagari(n_bytes=50000, seed=4):
    """Consonants with dependent vowel signs and viramas between them: the combining marks are neither letters nor
    digits, so they cut the words."""
    rng = np.random.default_rng(seed)
    cons = [chr(c) for c in range(0x915, 0x93A)]
    marks = [chr(c) for c in range(0x93E, 0x94E)] + ["ँ", "ं"]
    syll = [a + m for a in cons[:12] for m in marks[:6]] + cons
    return _words(int(rng.integers(1 << 30)), n_bytes, syll, extra=[" । ", "॥\n"], hi=5)


def digits(n_bytes=20000, seed=5):
    """Arabic-Indic and fullwidth digits in runs of 1 - 7."""
    pool = [chr(c) for c in range(0x660, 0x66A)] + [chr(c) for c in range(0xFF10, 0xFF1A)] + list("0123456789")
    return _words(seed, n_bytes, pool, extra=["x", "٫", "．"], hi=7)


def emoji(n_bytes=20000, seed=6):
    rng = np.random.default_rng(seed)
    faces = [chr(c) for c in range(0x1F600, 0x1F650)]
    out, size = [], 0
    while size < n_bytes:
        k = int(rng.integers(0, 5))
        a, b = faces[int(rng.integers(0, len(faces)))], faces[int(rng.integers(0, len(faces)))]
        w = [a, a + "\ufe0f", a + "\u200d" + b, "\u2764\ufe0f\u200d" + b, a + b + "\ufe0f"][k]
        w += [" ", "", " ok ", "\n", "!", " 1"][int(rng.integers(0, 6))]
        out.append(w)
        size += len(w.encode("utf-8"))
    return "".join(out).encode("utf-8")


WS = ["\u00a0", "\u2028", "\u0085", "\u3000", "\r", "\n", " ", " ", "\t", "\r\n"]


def whitespace(n_runs=3000, seed=7):
    """Whitespace runs of 1 - 6 characters of the four non-ASCII ones, CR / LF and spaces, in front of a letter, in
    front of a character that is neither letter nor digit nor whitespace, and at the end of the text."""
    rng = np.random.default_rng(seed)
    after = ["a", "\u00e9", "\u4e2d", "!", "\u3002", "\U0001f600", "'s", "7", "\uff17", "ab", ".."]
    before = ["a", "1", "\u4e2d", "!", "\u0301", "", "\uff17"]
    out = []
    for _ in range(n_runs):
        out.append(before[int(rng.integers(0, len(before)))] + _pick(rng, WS, int(rng.integers(1, 7))) +
                   after[int(rng.integers(0, len(after)))])
    return "".join(out).encode("utf-8") + _pick(rng, WS, 5).encode("utf-8")


def whitespace_ends(seed=8):
    """Short texts that end in such a run."""
    rng = np.random.default_rng(seed)
    return [(h + _pick(rng, WS, int(rng.integers(1, 6)))).encode("utf-8")
            for h in ("a", "中", "!", "1", "", "ab é") for _ in range(40)]


def pseudo_scripts():
    """name -> bytes"""
    return {"cjk": cjk(), "cyrillic": cyrillic(), "greek": greek(), "devanagari": devanagari(), "digits": digits(),
            "emoji": emoji(), "whitespace": whitespace()}


# a letter, whitespace and -- four bytes -- a symbol and a letter of 2, 3 and 4 bytes
ALIGN_CHARS = ["\u00e9", "\u00a0", "\u4e2d", "\u3000", "\U0001f600", "\U00020000"]


def alignment():
    """Every character of ALIGN_CHARS at every offset 0 .. 63 of a block (so at every offset of a 16-byte vector, and
    across the vector and block edges): first in the text, last in the text, right before and right after a sync point
    of either kind -> list of bytes."""
    texts = []
    for c in ALIGN_CHARS:
        texts.append((c + " ab cd " + c + c).encode("utf-8"))
        for off in range(BLOCK):
            fill = ("word " * 30)[:BLOCK + off - 1] + "a"           # ends on a letter; c starts at `off` of the 2nd block
            for tail in ("", " x", "\nq", "\n" + c, "'s", c + " " + c):
                texts.append((fill + c + tail).encode("utf-8"))
            fill = fill[:-2] + "b "                                  # c right behind a sync point (A) ...
            texts.append((fill + c + "z").encode("utf-8"))
            fill = fill[:-2] + ".\n"                                 # ... and (B)
            texts.append((fill + c + "z " + c).encode("utf-8"))
            fill = fill[:-3] + ".\u00a0"                            # a 2-byte whitespace that ends at the offset
            texts.append((fill + c + "z").encode("utf-8"))
    return texts


def max_span_texts(max_span=256):
    """(bytes, host spans expected) with one span of max_span - 1, max_span and max_span + 1 bytes whose last character
    straddles the limit or ends on it; a following ' b' makes the span end at a sync point instead of the text's end."""
    out = []
    for c in ("é", "中", "\U00020000"):
        k = len(c.encode("utf-8"))
        for n in (max_span - 1, max_span, max_span + 1):
            body = b"a" * (n - k) + c.encode("utf-8")
            out.append((body, int(n > max_span)))
            out.append((body + b" b", int(n > max_span)))
    return out


ILL_FORMED = [b"\x80", b"\xbf\xbf", b"\xc0\x80", b"\xc1\xbf", b"\xe0\x9f\xbf", b"\xed\xa0\x80", b"\xf4\x90\x80\x80",
              b"\xf5\x80\x80\x80", b"\xf8\x88\x80\x80\x80", b"\xfe", b"\xff", b"\xe4\xb8", b"\xf0\x9f\x98", b"\xc3",
              b"\xe4\xb8\xe4\xb8\xad", b"\xc3\xa9\xa9"]


def ill_formed():
    """-> list of (bytes, first bad byte, one past the last bad byte): each sequence of ILL_FORMED between clean spans, at
    every offset of a vector, and at the very end of a text (a sequence cut by the end of the text among them)."""
    out = []
    for bad in ILL_FORMED:
        for off in range(16):
            head = ("ab cd éf " * 4)[:30 + off].encode("utf-8", "ignore")
            head = head.decode("utf-8", "ignore").encode("utf-8") + b"g "
            for tail in (b" hi \xe4\xb8\xad jk", b"z\n\xe4\xb8\xad", b""):
                out.append((head + bad + tail, len(head), len(head) + len(bad)))
    return out
