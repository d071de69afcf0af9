"""Id matrices on the device (csrc/pack.hip) timed.  Every step below runs in a child process of its own under its own
time limit; when one fails, nothing after it is started.

  batch     shakespeare x --rep, every line a document (each line split by the gpt4 pattern on its own), golden gpt4
            model, text and matrix on the device: mbpe_encoder_kernel_ms of Encoder.encode_batch and, of the same call,
            the pack kernel alone (mbpe_encoder_pack_ms), as PADDED seq_len 64 and as PACKED seq_len 2,048, 32-bit ids.
  wide      the index-width case of tests/test_gpu_pack.py: 65,537 one-token documents at seq_len 65,536, 16 bits in
            and out, 8.6 GB (mbpe_pack_kernel_ms).
  route     wall clock for the 40,000 lines of one shakespeare: what a user had before -- Tokenizer.encode_batch, padding
            with numpy, upload -- against one Tokenizer.encode_batch_padded into device memory.

    python tools/pack_time.py --json profiles/r09_pack.json

With --aux, the training-batch outputs (k_pack_aux) instead, on the same two shapes -- PADDED seq_len 64 and PACKED
seq_len 2,048 over shakespeare x --rep, every line a document, 32-bit ids -- from the flat tokens in device memory
(one shakespeare encoded line by line, its tokens repeated on the device: every copy encodes alike).  Per layout:
  aux_all   (a) mbpe_pack_tokens_aux with labels, pos and seg, alternating with (c) the route a user has today: the three
            matrices built by torch ops on the device from the ids, the lengths and the uploaded offsets.  Kernel time
            of (a), wall clock of both, peak extra device memory of (c), and torch.equal of the results
  aux_ids   (b) mbpe_pack_tokens_aux with no output but ids and lengths, alternating with mbpe_pack_tokens (k_pack_padded
            / k_pack_stream): mbpe_pack_kernel_ms of both, and torch.equal of the matrices

    python tools/pack_time.py --aux --json profiles/r10_pack_aux.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SHAKESPEARE = os.path.join(ROOT, "tests", "golden", "data", "shakespeare.txt")
MODEL = os.path.join(ROOT, "tests", "golden", "shakespeare_gpt4_lexical_512.model")
PEAK_BYTES_PER_S = 8e12
PAD = 0

sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "minbpe-cc_amd", "python")]


def tiled(one, step, rep):
    """Offsets of `rep` copies of a text: one copy's offsets `one` (from 0 to step), repeated."""
    import numpy as np
    off = np.empty(rep * (len(one) - 1) + 1, dtype=np.uint64)
    off[0] = 0
    body = one[1:].astype(np.uint64)
    k = len(body)
    for r in range(rep):
        off[1 + r * k:1 + (r + 1) * k] = body + np.uint64(r * step)
    return off


def pack_bytes(lengths_sum, n_rows, n_docs, seq_len, nbe, token_bytes, id_bytes):
    """Bytes the pack kernel reads and writes, as it is written: every token that lands in a row once, the document
    offsets once; every id and every length once."""
    read = (lengths_sum - nbe * n_docs) * token_bytes + (n_docs + 1) * 8
    written = n_rows * seq_len * id_bytes + n_rows * 4
    return read, written


def step_batch(args):
    import numpy as np
    import torch
    import mbpe
    import oracle as O
    dev = torch.device("cuda", 0)
    sh = open(SHAKESPEARE, "rb").read()
    lines = sh.splitlines(keepends=True)
    merges = O.parse_model(open(MODEL, "rb").read())[2]
    pattern = mbpe.split_pattern("gpt4")
    parts, first, at = [], [0], 0
    for x in lines:                                                    # every line split on its own
        o = mbpe.presplit(pattern, x)
        parts.append(o[1:] + np.uint64(at))
        at += len(x)
        first.append(first[-1] + len(o) - 1)
    one_off = np.concatenate([[0]] + parts).astype(np.uint64)
    one_doc = np.array(first, dtype=np.uint64)
    rep = args.rep
    text = torch.from_numpy(np.frombuffer(sh, dtype=np.uint8).copy()).to(dev).repeat(rep)
    off = tiled(one_off, len(sh), rep)
    docs = tiled(one_doc, len(one_off) - 1, rep)
    torch.cuda.synchronize()
    res = {"device": torch.cuda.get_device_name(0), "lib": mbpe.lib().mbpe_version().decode(), "rep": rep,
           "text_bytes": text.numel(), "chunks": len(off) - 1, "documents": len(docs) - 1, "cases": []}
    with mbpe.Encoder(merges) as enc:
        for layout, seq_len in (("padded", 64), ("packed", 2048)):
            kw = dict(seq_len=seq_len, layout=layout, out_bits=32, pad_id=PAD, text_ptr=text.data_ptr(), n_bytes=text.numel())
            ids, lengths = enc.encode_batch(None, off[:len(one_off)], docs[:len(one_doc)], **dict(kw, n_bytes=len(sh)))
            n_rows = len(ids) * rep if layout == "padded" else -(-int(lengths.sum()) * rep // seq_len)
            d_ids = torch.empty((n_rows, seq_len), dtype=torch.int32, device=dev)
            d_len = torch.empty(n_rows, dtype=torch.int32, device=dev)
            total, pack, wall = [], [], []
            torch.cuda.synchronize()                                   # (the encoder works on a stream of its own)
            for i in range(1 + args.reps):
                t = time.perf_counter()
                got = enc.encode_batch(None, off, docs, out_ptr=d_ids.data_ptr(), len_ptr=d_len.data_ptr(),
                                       cap_rows=n_rows, **kw)
                w = time.perf_counter() - t
                assert got == n_rows
                if i:
                    total.append(enc.kernel_ms()); pack.append(enc.pack_ms()); wall.append(w)
            if layout == "padded":                                     # every copy is the first one
                assert bool((d_ids.view(rep, -1) == torch.from_numpy(ids.view(np.int32)).to(dev).view(1, -1)).all())
            len_sum = int(d_len.sum(dtype=torch.int64))
            read, written = pack_bytes(len_sum, n_rows, len(docs) - 1, seq_len, 0, 4, 4)
            p = statistics.median(pack)
            res["cases"].append({
                "layout": layout, "seq_len": seq_len, "out_bits": 32, "rows": n_rows, "tokens": enc.n_tokens,
                "ids_from_tokens": len_sum, "kernel_ms": total, "pack_ms": pack, "call_wall_s": wall,
                "kernel_ms_median": statistics.median(total), "pack_ms_median": p,
                "pack_share_of_encode_passes": p / (statistics.median(total) - p),
                "bytes_read": read, "bytes_written": written, "GBps": (read + written) / p / 1e6,
                "share_of_8TBps": (read + written) / (p * 1e-3) / PEAK_BYTES_PER_S})
            del d_ids, d_len
            torch.cuda.empty_cache()
    print(json.dumps(res))


def step_wide(args):
    import numpy as np
    import torch
    import mbpe
    dev = torch.device("cuda", 0)
    n_docs, seq_len = 65537, 65536
    tokens = torch.from_numpy(np.random.default_rng(1).integers(0, 40000, size=n_docs, dtype=np.uint16).view(np.int16)).to(dev)
    off = np.arange(n_docs + 1, dtype=np.uint64)
    out = torch.empty((n_docs, seq_len), dtype=torch.int16, device=dev)
    lengths = torch.empty(n_docs, dtype=torch.int32, device=dev)
    ms = []
    torch.cuda.synchronize()
    for i in range(1 + args.reps):
        n = mbpe.pack_tokens(None, off, seq_len, "padded", 16, 7, tokens_ptr=tokens.data_ptr(), n_tokens=n_docs, token_bits=16,
                             out_ptr=out.data_ptr(), len_ptr=lengths.data_ptr(), cap_rows=n_docs)
        assert n == n_docs
        if i:
            ms.append(mbpe.pack_kernel_ms())
    assert bool(torch.equal(out[:, 0], tokens)) and bool((out[-1, 1:] == 7).all()) and bool((lengths == 1).all())
    read, written = pack_bytes(n_docs, n_docs, n_docs, seq_len, 0, 2, 2)
    p = statistics.median(ms)
    print(json.dumps({"documents": n_docs, "seq_len": seq_len, "out_bits": 16, "pack_ms": ms, "pack_ms_median": p,
                      "bytes_read": read, "bytes_written": written, "GBps": (read + written) / p / 1e6,
                      "share_of_8TBps": (read + written) / (p * 1e-3) / PEAK_BYTES_PER_S}))


def step_route(args):
    import numpy as np
    import torch
    import mbpe
    import oracle as O
    dev = torch.device("cuda", 0)
    lines = open(SHAKESPEARE, "rb").read().splitlines(keepends=True)
    tok = mbpe.Tokenizer(O.GPT4_SPLIT_PATTERN)
    tok.set_merges(O.parse_model(open(MODEL, "rb").read())[2])
    seq_len = 64

    def before():
        enc = tok.encode_batch(lines, device=0)
        ids = np.full((len(enc), seq_len), PAD, dtype=np.uint32)
        lengths = np.zeros(len(enc), dtype=np.uint32)
        for i, e in enumerate(enc):
            n = min(len(e), seq_len)
            ids[i, :n] = e[:n]
            lengths[i] = n
        d = torch.from_numpy(ids.view(np.int32)).to(dev), torch.from_numpy(lengths.view(np.int32)).to(dev)
        torch.cuda.synchronize()
        return d

    d_ids = torch.empty((len(lines), seq_len), dtype=torch.int32, device=dev)
    d_len = torch.empty(len(lines), dtype=torch.int32, device=dev)

    def now():
        tok.encode_batch_padded(lines, seq_len, pad_id=PAD, out_ptr=d_ids.data_ptr(), len_ptr=d_len.data_ptr(),
                                cap_rows=len(lines))
        torch.cuda.synchronize()

    a, b = [], []
    torch.cuda.synchronize()
    for i in range(1 + args.reps):
        t = time.perf_counter(); want = before(); ta = time.perf_counter() - t
        t = time.perf_counter(); now(); tb = time.perf_counter() - t
        if i:
            a.append(ta); b.append(tb)
    assert bool(torch.equal(want[0], d_ids)) and bool(torch.equal(want[1], d_len))
    print(json.dumps({"documents": len(lines), "seq_len": seq_len, "encode_batch_numpy_upload_s": a,
                      "encode_batch_padded_s": b, "encode_batch_numpy_upload_s_median": statistics.median(a),
                      "encode_batch_padded_s_median": statistics.median(b)}))


AUX_SHAPES = {"padded": 64, "packed": 2048}
IGNORE = -100


def aux_setup(args):
    """-> (dev, flat tokens on the device, doc_tok_off, facts): shakespeare x rep, every line a document."""
    import numpy as np
    import torch
    import mbpe
    import oracle as O
    dev = torch.device("cuda", 0)
    lines = open(SHAKESPEARE, "rb").read().splitlines(keepends=True)
    tok = mbpe.Tokenizer(O.GPT4_SPLIT_PATTERN)
    tok.set_merges(O.parse_model(open(MODEL, "rb").read())[2])
    enc = tok.encode_batch(lines, device=0)
    tok.close()
    flat = np.concatenate(enc).astype(np.uint32)
    one_off = np.concatenate([[0], np.cumsum([len(e) for e in enc])]).astype(np.uint64)
    off = tiled(one_off, len(flat), args.rep)
    tokens = torch.from_numpy(flat.view(np.int32)).to(dev).repeat(args.rep)
    torch.cuda.synchronize()
    facts = {"device": torch.cuda.get_device_name(0), "lib": mbpe.lib().mbpe_version().decode(), "rep": args.rep,
             "layout": args.layout, "seq_len": AUX_SHAPES[args.layout], "out_bits": 32, "tokens": tokens.numel(),
             "documents": len(off) - 1, "longest_document": int(np.diff(one_off.astype(np.int64)).max())}
    return dev, tokens, off, facts


def aux_rows(tokens, off, seq_len, layout):
    """The row count of the matrix: the query of mbpe_pack_tokens (no device work)."""
    import ctypes
    import mbpe
    spec = mbpe.pack_spec(seq_len, layout, 32, PAD)
    n_rows = ctypes.c_uint64()
    rc = mbpe.lib().mbpe_pack_tokens(0, ctypes.c_void_p(tokens.data_ptr()), tokens.numel(), 32, 1, off.ctypes.data,
                                     len(off) - 1, ctypes.byref(spec), None, 0, 1, None, ctypes.byref(n_rows))
    assert rc == mbpe.OK, rc
    return n_rows.value


def torch_route(torch, ids, lengths, off_host, packed):
    """What a user builds today from the packed ids, the lengths and the host's offsets -> (labels, pos, seg), int32."""
    dev = ids.device
    n_rows, seq_len = ids.shape
    if not packed:                                                   # right-padded rows: a column mask
        col = torch.arange(seq_len, dtype=torch.int32, device=dev)
        mask = col[None, :] < lengths[:, None]
        pos = torch.where(mask, col[None, :], 0).to(torch.int32)
        seg = torch.where(mask, torch.arange(1, n_rows + 1, dtype=torch.int32, device=dev)[:, None], 0).to(torch.int32)
    else:                                                            # the cell's document by a search in the offsets
        off = torch.from_numpy(off_host.view("int64")).to(dev)
        f = torch.arange(n_rows * seq_len, dtype=torch.int64, device=dev)
        d = torch.searchsorted(off[1:], f, right=True)               # (the first document that ends behind f)
        live = f < off[-1]
        d.clamp_(max=off.numel() - 2)
        pos = torch.where(live, f - off[d], 0).to(torch.int32).view(n_rows, seq_len)
        seg = torch.where(live, d + 1, 0).to(torch.int32).view(n_rows, seq_len)
    # the usual shift by one column: the last column has no target
    labels = torch.full_like(ids, IGNORE)
    same = (seg[:, 1:] == seg[:, :-1]) & (seg[:, 1:] != 0)
    labels[:, :-1] = torch.where(same, ids[:, 1:], IGNORE)
    return labels, pos, seg


def step_aux_all(args):
    import torch
    import mbpe
    dev, tokens, off, res = aux_setup(args)
    layout, seq_len = args.layout, AUX_SHAPES[args.layout]
    kw = dict(tokens_ptr=tokens.data_ptr(), n_tokens=tokens.numel(), token_bits=32)
    n_rows = aux_rows(tokens, off, seq_len, layout)
    ids, lab, pos, seg = (torch.empty((n_rows, seq_len), dtype=torch.int32, device=dev) for _ in range(4))
    lengths = torch.empty(n_rows, dtype=torch.int32, device=dev)

    def ours():
        got = mbpe.pack_tokens_aux(None, off, seq_len, layout, 32, PAD, out_ptr=ids.data_ptr(), len_ptr=lengths.data_ptr(),
                                   cap_rows=n_rows, labels_ptr=lab.data_ptr(), pos_ptr=pos.data_ptr(),
                                   seg_ptr=seg.data_ptr(), ignore_label=IGNORE, **kw)
        assert got == n_rows
        return mbpe.pack_kernel_ms()

    ms, wall_a, wall_c, peak = [], [], [], []
    torch.cuda.synchronize()
    for i in range(1 + args.reps):
        t = time.perf_counter(); k = ours(); torch.cuda.synchronize(); ta = time.perf_counter() - t
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        t = time.perf_counter()
        want = torch_route(torch, ids, lengths, off, layout == "packed")
        torch.cuda.synchronize()
        tc = time.perf_counter() - t
        extra = torch.cuda.max_memory_allocated() - base - sum(w.numel() * 4 for w in want)
        if i:
            ms.append(k); wall_a.append(ta); wall_c.append(tc); peak.append(extra)
        if i < args.reps:
            del want
            torch.cuda.empty_cache()
    cols = slice(None, -1) if layout == "packed" else slice(None)
    res.update({
        "rows": n_rows, "cells": n_rows * seq_len,
        "aux_kernel_ms": ms, "aux_kernel_ms_median": statistics.median(ms),
        "aux_wall_s": wall_a, "aux_wall_s_median": statistics.median(wall_a),
        "torch_wall_s": wall_c, "torch_wall_s_median": statistics.median(wall_c),
        "torch_peak_extra_bytes": max(peak), "result_bytes_three_matrices": 3 * n_rows * seq_len * 4,
        "pos_equal": bool(torch.equal(want[1], pos)), "seg_equal": bool(torch.equal(want[2], seg)),
        "labels_equal_compared_columns": "all but the last" if layout == "packed" else "all",
        "labels_equal": bool(torch.equal(want[0][:, cols], lab[:, cols])),
        "last_column_labels_that_differ": int((want[0][:, -1] != lab[:, -1]).sum()),
        "bytes_written": n_rows * seq_len * 16 + n_rows * 4,
        "bytes_read": int(lengths.sum(dtype=torch.int64)) * 4 + len(off) * 8})
    res["GBps"] = (res["bytes_read"] + res["bytes_written"]) / res["aux_kernel_ms_median"] / 1e6
    res["share_of_8TBps"] = res["GBps"] * 1e9 / PEAK_BYTES_PER_S
    assert res["pos_equal"] and res["seg_equal"] and res["labels_equal"], res
    print(json.dumps(res))


def step_aux_ids(args):
    import torch
    import mbpe
    dev, tokens, off, res = aux_setup(args)
    layout, seq_len = args.layout, AUX_SHAPES[args.layout]
    kw = dict(tokens_ptr=tokens.data_ptr(), n_tokens=tokens.numel(), token_bits=32)
    n_rows = aux_rows(tokens, off, seq_len, layout)
    old_ids, new_ids = (torch.empty((n_rows, seq_len), dtype=torch.int32, device=dev) for _ in range(2))
    old_len, new_len = (torch.empty(n_rows, dtype=torch.int32, device=dev) for _ in range(2))
    old, new = [], []
    torch.cuda.synchronize()
    for i in range(1 + args.reps):
        assert mbpe.pack_tokens(None, off, seq_len, layout, 32, PAD, out_ptr=old_ids.data_ptr(), len_ptr=old_len.data_ptr(),
                                cap_rows=n_rows, **kw) == n_rows
        a = mbpe.pack_kernel_ms()
        assert mbpe.pack_tokens_aux(None, off, seq_len, layout, 32, PAD, out_ptr=new_ids.data_ptr(),
                                    len_ptr=new_len.data_ptr(), cap_rows=n_rows, **kw) == n_rows
        b = mbpe.pack_kernel_ms()
        if i:
            old.append(a); new.append(b)
    assert bool(torch.equal(old_ids, new_ids)) and bool(torch.equal(old_len, new_len))
    res.update({"rows": n_rows, "cells": n_rows * seq_len, "pack_tokens_kernel_ms": old, "aux_ids_only_kernel_ms": new,
                "pack_tokens_kernel_ms_median": statistics.median(old),
                "aux_ids_only_kernel_ms_median": statistics.median(new), "ids_and_lengths_equal": True})
    print(json.dumps(res))


STEPS = {"batch": step_batch, "wide": step_wide, "route": step_route, "aux_all": step_aux_all, "aux_ids": step_aux_ids}


def child(step, limit, extra):
    """One step in a fresh process under its own time limit -> its JSON line, or None (and nothing more is run)."""
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step] + extra
    print("+", " ".join(cmd), flush=True)
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT)
    if p.returncode != 0:
        print("step %s ended with status %d\n%s" % (step, p.returncode, p.stderr[-4000:]), flush=True)
        return None
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEPS))
    ap.add_argument("--rep", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json")
    ap.add_argument("--aux", action="store_true", help="the k_pack_aux rows instead of the r09 steps")
    ap.add_argument("--layout", choices=sorted(AUX_SHAPES), default="padded")
    args = ap.parse_args()
    if args.step:
        STEPS[args.step](args)
        return 0
    res = {}
    size = ["--rep", str(args.rep), "--reps", str(args.reps)]
    plan = [("route", "route", 200, size), ("wide", "wide", 200, size), ("batch", "batch", 500, size)]
    if args.aux:
        plan = [("%s_%s" % (step, layout), step, 240, size + ["--layout", layout])
                for layout in ("padded", "packed") for step in ("aux_all", "aux_ids")]
    for name, step, limit, extra in plan:
        res[name] = child(step, limit, extra)
        if res[name] is None:
            break
        print(json.dumps(res[name]), flush=True)
        if args.json:
            with open(args.json, "w") as f:
                json.dump(res, f, indent=1)
    return 0 if all(res.get(name) is not None for name, *_ in plan) else 1


if __name__ == "__main__":
    sys.exit(main())
