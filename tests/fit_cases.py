"""The judge of the fit layout (mbpe_pack_fit): ref_fit builds every row from Python lists, straight from the rule in
include/mbpe.h, and shares no code with the library.  ref_fit_naive is the same rule with a scan over all open rows
per piece; test_pack_fit_cpu.py holds the two equal.  Used by test_pack_fit_cpu.py, test_gpu_pack_fit.py and
test_gpu_encode_fit.py."""
import bisect

NO_ROW = (1 << 64) - 1


def _elements(docs, bos, eos):
    return [([bos] if bos is not None else []) + [int(t) for t in tok] + ([eos] if eos is not None else []) for tok in docs]


def _pieces(T, seq_len):
    """T: the documents' element counts -> the pieces (size, d, i) in placement order."""
    S = seq_len
    pieces = []
    for d, n in enumerate(T):
        q, r = divmod(n, S)
        pieces += [(S, d, i) for i in range(q)]
        if r:
            pieces.append((r, d, q))
    pieces.sort(key=lambda p: (-p[0], p[1], p[2]))
    return pieces


def ref_plan(T, seq_len):
    """T: the documents' element counts -> (placed: (row, col0, size, d, i) per piece in placement order, n_rows).  The
    open rows are a sorted list of (free, row); bisect finds the smallest free that holds the piece, then the lowest
    row."""
    S = seq_len
    open_rows = []                                   # sorted (free, row), free > 0
    placed, n_rows = [], 0
    for size, d, i in _pieces(T, S):
        at = bisect.bisect_left(open_rows, (size, -1))
        if at < len(open_rows):
            free, row = open_rows.pop(at)
        else:
            free, row = S, n_rows
            n_rows += 1
        placed.append((row, S - free, size, d, i))
        if free > size:
            bisect.insort(open_rows, (free - size, row))
    return placed, n_rows


def plan_outputs(placed, n_rows, n_docs):
    """-> (len per row, doc_row, doc_col) of a placement."""
    length, doc_row, doc_col, last = [0] * n_rows, [NO_ROW] * n_docs, [0] * n_docs, [-1] * n_docs
    for row, col0, size, d, i in placed:
        assert col0 == length[row]                   # a row fills from the left, without a gap
        length[row] += size
        if i > last[d]:
            last[d], doc_row[d], doc_col[d] = i, row, col0
    return length, doc_row, doc_col


def _build(E, placed, n_rows, seq_len, pad, ignore):
    """placed: (row, col0, size, d, i) per piece -> the dict of lists."""
    S = seq_len
    out = {"ids": [[pad] * S for _ in range(n_rows)], "labels": [[ignore] * S for _ in range(n_rows)],
           "pos": [[0] * S for _ in range(n_rows)], "seg": [[0] * S for _ in range(n_rows)], "len": [0] * n_rows,
           "doc_row": [NO_ROW] * len(E), "doc_col": [0] * len(E)}
    last = {}
    for row, col0, size, d, i in placed:
        e = E[d]
        for t in range(size):
            k = i * S + t
            assert out["seg"][row][col0 + t] == 0
            out["ids"][row][col0 + t] = e[k]
            out["labels"][row][col0 + t] = e[k + 1] if k + 1 < len(e) else ignore
            out["pos"][row][col0 + t] = k
            out["seg"][row][col0 + t] = d + 1
        out["len"][row] += size
        if d not in last or i > last[d][0]:
            last[d] = (i, row, col0)
    for d, (_, row, col0) in last.items():
        out["doc_row"][d], out["doc_col"][d] = row, col0
    return out


def ref_fit(docs, seq_len, bos, eos, pad, ignore):
    """docs: a list of token lists; bos / eos None = not set -> a dict of lists: "ids", "labels", "pos", "seg" (one list
    of seq_len per row), "len" (one entry per row), "doc_row", "doc_col" (one entry per document)."""
    E = _elements(docs, bos, eos)
    placed, n_rows = ref_plan([len(e) for e in E], seq_len)
    return _build(E, placed, n_rows, seq_len, pad, ignore)


def ref_fit_naive(docs, seq_len, bos, eos, pad, ignore):
    """The same rule, quadratic: every piece looks at every row opened so far."""
    S = seq_len
    E = _elements(docs, bos, eos)
    free = []                                        # per row
    placed = []
    for size, d, i in _pieces([len(e) for e in E], S):
        best = None
        for row, f in enumerate(free):
            if f >= size and (best is None or f < free[best]):
                best = row
        if best is None:
            best = len(free)
            free.append(S)
        placed.append((best, S - free[best], size, d, i))
        free[best] -= size
    return _build(E, placed, len(free), S, pad, ignore)


def cu_of(ref, seq_len):
    """cu_seqlens and max_seqlen from ref_fit's seg matrix: the boundaries of the maximal runs of equal (row, seg)."""
    cu, longest = [0], 0
    for r, seg in enumerate(ref["seg"]):
        for c in range(1, seq_len):
            if seg[c] != seg[c - 1]:
                cu.append(r * seq_len + c)
        cu.append((r + 1) * seq_len)
    for a, b in zip(cu, cu[1:]):
        longest = max(longest, b - a)
    return cu, longest


def grid_lengths(seq_len, nbe):
    """About 40 document lengths on the grid of the rule's edges -- 0, 1, one below a full row, a full row, one above,
    two rows, three rows and one -- with fillers between them and runs of empty documents at the start, in the
    middle and at the end."""
    S = seq_len
    edges = [0, 1, max(S - nbe - 1, 0), max(S - nbe, 0), S - nbe + 1, 2 * S, 3 * S + 1]
    lens = [0, 0, 0]
    for k, e in enumerate(edges):
        lens += [e, 1 if k % 2 else max(S // 2, 1)]
    lens += [0, 0, 0, 0]
    for k, e in enumerate(reversed(edges)):
        lens += [e, (k * 3) % (S + 2), 0 if k % 2 else 2]
    lens += [0, 0]
    return lens
