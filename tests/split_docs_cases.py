"""Documents, names and the truth for the tests of mbpe_splitter_split_docs (test_split_docs_cpu.py,
test_gpu_split_docs.py): a Python restatement of Tokenizer::split_on_special gives the pieces of every document, and
mbpe_presplit (split_cases.truth_end_mask) splits every piece that is not a range as a text of its own."""
import numpy as np

import split_cases as S

RAW = 0xFFFFFFFF            # MBPE_SPLIT_RAW


def join(docs):
    """list of bytes -> (uint8 blob, uint64 offsets [n_docs + 1])."""
    off = np.zeros(len(docs) + 1, dtype=np.uint64)
    np.cumsum([len(d) for d in docs], out=off[1:])
    return np.frombuffer(b"".join(docs), dtype=np.uint8), off


def plan(blob, off, names):
    """split_on_special of every document blob[off[i]:off[i + 1]] -> (piece boundaries b, ascending and distinct,
    piece k = [b[k], b[k + 1]); ranges as int64 [n_ranges, 3] rows (start, len, name index or RAW))."""
    data = np.asarray(blob, dtype=np.uint8).tobytes()
    off = np.asarray(off, dtype=np.int64)
    occ = []
    for k, name in enumerate(names):
        if not name:
            continue
        p = data.find(name)
        while p >= 0:
            occ.append((p, k))
            p = data.find(name, p + 1)
    occ.sort()                                                     # by (position, name index)
    taken = []
    cursor = 0
    for p, k in occ:
        doc_end = int(off[np.searchsorted(off, p, side="right")])
        if p + len(names[k]) > doc_end:                            # straddles two documents: no occurrence
            continue
        if p < cursor:                                             # inside one already taken (the cursor never passes
            continue                                               # a document's end, so it need not be reset)
        taken.append((p, len(names[k]), k))
        cursor = p + len(names[k])
    marks = [off] + [np.array([p for p, _, _ in taken] + [p + n for p, n, _ in taken], dtype=np.int64)]
    b = np.unique(np.concatenate(marks))
    is_taken = {p: k for p, _, k in taken}
    rows = []
    arr = np.asarray(blob, dtype=np.uint8)
    for a, e in zip(b[:-1].tolist(), b[1:].tolist()):
        if a in is_taken:
            rows.append((a, e - a, is_taken[a]))
        elif arr[a] == 0:
            rows.append((a, e - a, RAW))
    return b, np.array(rows, dtype=np.int64).reshape(len(rows), 3)


def truth(pattern, blob, off, names):
    """-> (bool[len(blob)] True where a byte is the last of its chunk, ranges [n_ranges, 3], piece boundaries)."""
    b, ranges = plan(blob, off, names)
    if len(blob) == 0:
        return np.zeros(0, dtype=bool), ranges, b
    mask = S.truth_end_mask(pattern, blob, b)
    for a, n, _ in ranges.tolist():                                # a range is one chunk
        mask[a:a + n] = False
        mask[a + n - 1] = True
    return mask, ranges, b


def string_sets(n_strings=200000):
    """n_strings random strings of 0 .. 40 characters from HOSTILE, ASCII and ASCII + NON_ASCII as documents: cuts on
    every residue mod 16 and mod 64."""
    each = n_strings // 3
    parts = [S.random_strings(41, n_strings - 2 * each, 40, S.HOSTILE),
             S.random_strings(42, each, 40, S.ASCII),
             S.random_strings(43, each, 40, S.ASCII, S.NON_ASCII, 0.08)]
    blob = np.concatenate([p[0] for p in parts])
    off = [np.zeros(1, dtype=np.uint64)]
    base = 0
    for data, o in parts:
        off.append(o[1:] + np.uint64(base))
        base += len(data)
    return blob, np.concatenate(off)


E = b"<|endoftext|>"

# (id, documents, names)
NAMED = [
    ("pair", [b"a  ", b"b", b"a \r\n", b"b", b"a\r\n ", b"b", b"a\n\n", b"\nb", b"a \n", b" b", b"a\r", b"\nb", b"a  b"], []),
    ("long whitespace", [b"ab" + b" " * 65, b"x", b"cd" + b" \n" * 40, b"y", b" " * 130, b"\t" * 64 + b"q",
                         b"z" + b"\r\n" * 70, b" k"], []),
    ("empty documents", [b"", b"", b"abc def", b"", b"", b"ghi  ", b"", b""], []),
    ("cut at a sync point", [b"hello", b" world", b"ab1", b"\n\nxy", b"it", b"'s", b"x" * 63 + b"a", b" b"], []),
    ("prefix, short first", [b"x<|a|>by <|a|>", b"<|a|>b<|a|>"], [b"<|a|>", b"<|a|>b"]),
    ("prefix, long first", [b"x<|a|>by <|a|>", b"<|a|>b<|a|>"], [b"<|a|>b", b"<|a|>"]),
    ("overlap", [b"zabcd abcdbcd", b"bcdabc"], [b"abc", b"bcd"]),
    ("adjacent", [b"<e><e><e>x<e>", b"a <e><e> b"], [b"<e>"]),
    ("first and last byte", [b"<e>middle<e>", b"<e>", b"<e> x", b"x <e>"], [b"<e>"]),
    ("straddle", [b"ab<", b"e>cd", b"x<e", b">", b"<e>"], [b"<e>"]),
    ("non-ascii name", ["a<é>b中c 中".encode(), "中é<é>".encode()],
     ["<é>".encode(), "中".encode()]),
    ("space and letter", [b"a tok b Wordy tokWord  tok", b" tok", b"Word"], [b" tok", b"Word"]),
    ("nul-led parts", [b"\x00123", b"\x00abc def", b"x<e>\x0042<e>\x00 7 z", b"\x00", b"a\x00b", b"<e>\x00-5"], [b"<e>"]),
    ("empty name", [b"a<e>b"], [b"", b"<e>"]),
    ("endoftext", [b"First doc." + E + b"Second  " + E + E + b" third\n", E, b"no special here  "], [E]),
]
