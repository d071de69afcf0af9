"""The judge of the window layout (mbpe_pack_windows): ref_windows builds every row from Python lists, straight from
the rule in include/mbpe.h, and shares no code with the library.  Used by test_pack_windows_cpu.py,
test_gpu_pack_windows.py and test_gpu_encode_windows.py."""


def ref_windows(docs, seq_len, stride, bos, eos, pad, ignore, score_once):
    """docs: a list of token lists; bos / eos None = not set -> a dict of lists: "ids", "labels", "pos", "seg" (one
    list of seq_len per row), "len", "row_doc", "row_tok0" (one entry per row)."""
    nb, ne = int(bos is not None), int(eos is not None)
    keep = seq_len - nb - ne
    step = keep - stride
    assert keep >= 1 and 0 <= stride < keep
    out = {k: [] for k in ("ids", "labels", "pos", "seg", "len", "row_doc", "row_tok0")}
    for d, tok in enumerate(docs):
        tok = [int(t) for t in tok]
        L = len(tok)
        W = 1 if L <= keep else 1 + -((keep - L) // step)        # 1 + ceil((L - keep) / step)
        # what follows token index t - 1 in the document: the targets, eos behind the last token
        target = lambda t: tok[t] if t < L else (eos if ne and t == L else ignore)
        for i in range(W):
            a = i * step
            b = min(a + keep, L)
            last = i == W - 1
            ids, labels = [], []
            if nb:
                ids.append(bos)
                labels.append(target(a))
            for t in range(a, b):
                ids.append(tok[t])
                labels.append(target(t + 1))
            if score_once and i >= 1:
                for c in range(nb + stride):
                    labels[c] = ignore
            if ne and last:
                ids.append(eos)
                labels.append(ignore)
            n = len(ids)
            assert n == nb + (b - a) + (ne and last) and n <= seq_len
            out["ids"].append(ids + [pad] * (seq_len - n))
            out["labels"].append(labels + [ignore] * (seq_len - n))
            out["pos"].append(list(range(n)) + [0] * (seq_len - n))
            out["seg"].append([d + 1] * n + [0] * (seq_len - n))
            out["len"].append(n)
            out["row_doc"].append(d)
            out["row_tok0"].append(a)
        if L > keep:                                             # the last window brings a token no earlier one held
            assert (W - 2) * step + keep < L <= (W - 1) * step + keep
    return out


def ref_padded(docs, seq_len, bos, eos, pad, ignore):
    """MBPE_PACK_PADDED with pad_left = trunc_left = 0 and its labels, positions and segments, row by row: E_d = [bos]
    body [eos], labels E_d[k + 1], never across a document."""
    nb, ne = int(bos is not None), int(eos is not None)
    out = {k: [] for k in ("ids", "labels", "pos", "seg", "len")}
    for d, tok in enumerate(docs):
        E = ([bos] if nb else []) + [int(t) for t in tok][:seq_len - nb - ne] + ([eos] if ne else [])
        n = len(E)
        out["ids"].append(E + [pad] * (seq_len - n))
        out["labels"].append(E[1:] + [ignore] * (seq_len - n + (1 if n else 0)))
        out["pos"].append(list(range(n)) + [0] * (seq_len - n))
        out["seg"].append([d + 1] * n + [0] * (seq_len - n))
        out["len"].append(n)
    return out


def scored(ref, ignore):
    """Per document, in row order: the labels of ref_windows' rows that are not `ignore`."""
    per_doc = {}
    for row, d in enumerate(ref["row_doc"]):
        per_doc.setdefault(d, []).extend(v for v in ref["labels"][row] if v != ignore)
    return per_doc


def grid_lengths(keep, step):
    """The document lengths of the exact grid: every edge of the window count, a long document, and runs of empty
    documents at the start, in the middle and at the end; one-row documents between the long ones."""
    edges = [0, 1, keep - 1, keep, keep + 1, keep + step - 1, keep + step, keep + step + 1, 3000]
    lens = [0, 0, 0]
    for k, e in enumerate(edges):
        lens += [e, 1 if k % 2 else keep]                        # a one-row document behind each
    lens += [0, 0, 0, 0]
    for e in reversed(edges):
        lens += [e, 0 if e % 2 else 2]
    lens += [0, 0]
    return lens
