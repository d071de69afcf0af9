"""Best-fit packing (mbpe_pack_fit, csrc/pack_fit.h, k_pack_fit) timed: the figures of profiles/r27_pack_fit.md.  Every
step below runs in a child process of its own under its own time limit; when one fails, nothing after it is started.

  long      1,000 documents of 600,000 tokens in rows of 512 (the long workload of profiles/r25_pack_windows.md)
  short     1,000,000 documents of 1 .. 1,024 tokens (uniform) in rows of 2,048
            Per workload, 32-bit tokens in device memory, no bos / eos, all outputs in device memory: the planner alone
            by the host clock (mbpe_pack_fit_plan); rows and pad share of fit, PADDED and PACKED and the share of
            documents PADDED truncates and PACKED cuts; mbpe_pack_kernel_ms of mbpe_pack_fit with all four matrices,
            alternating with mbpe_pack_tokens_aux PACKED (k_pack_aux) on the same tokens, and per cell written; the
            wall clock of both calls; k_pack_fit with ids and lengths alone; short only: the documents' offsets from the
            device to the host, what the encoder calls add.
  existing  with --parent-root (a checkout of the parent commit with its library built): PADDED, PACKED and windows
            kernel times over 250,000 documents of 1 .. 1,024 tokens, this tree and the parent alternately, two
            processes each.

    python tools/pack_fit_time.py [--parent-root DIR]
"""
import argparse
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIMIT = 180


def med(xs):
    xs = sorted(xs)
    return "%.3f (%.3f-%.3f)" % (xs[len(xs) // 2], xs[0], xs[-1])


def workload(which):
    import numpy as np
    if which == "long":
        return 512, np.full(1000, 600000, dtype=np.int64)
    return 2048, np.random.default_rng(1).integers(1, 1025, 1000000)


def step_fit(which):
    import numpy as np
    import torch
    import mbpe
    dev = torch.device("cuda", 0)
    S, lens = workload(which)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    n_tok, n_docs = int(off[-1]), len(lens)
    d_tok = (torch.arange(n_tok, dtype=torch.int32, device=dev) % 60000) + 10
    torch.cuda.synchronize()
    print(which, "documents", n_docs, "tokens", n_tok, "seq_len", S, mbpe.lib().mbpe_version().decode())
    ts = []
    for _ in range(3):
        t = time.perf_counter()
        plan = mbpe.pack_fit_plan(off, S)
        ts.append((time.perf_counter() - t) * 1e3)
    n_fit = plan["n_rows"]
    n_packed = -(-n_tok // S)
    print("planner ms", med(ts))
    print("rows: fit %d, padded %d, packed %d" % (n_fit, n_docs, n_packed))
    print("pad share: fit %.5f, padded %.5f, packed %.6f" % (1 - n_tok / (n_fit * S), 1 - np.minimum(lens, S).sum() / (n_docs * S),
                                                            1 - n_tok / (n_packed * S)))
    starts, ends = off[:-1].astype(np.int64), off[1:].astype(np.int64)
    print("documents: padded truncates %.4f, packed cuts %.4f, fit cuts %.4f" %
          ((lens > S).mean(), ((ends - 1) // S != starts // S).mean(), (lens > S).mean()))
    n_max = max(n_fit, n_packed)
    ids, lab, pos, seg = (torch.empty(n_max * S, dtype=torch.int32, device=dev) for _ in range(4))
    ln = torch.empty(n_max, dtype=torch.int32, device=dev)
    d_row = torch.empty(n_docs, dtype=torch.int64, device=dev)
    d_col = torch.empty(n_docs, dtype=torch.int32, device=dev)
    common = dict(tokens_ptr=d_tok.data_ptr(), n_tokens=n_tok, token_bits=32)
    ptrs = dict(out_ptr=ids.data_ptr(), len_ptr=ln.data_ptr(), labels_ptr=lab.data_ptr(), pos_ptr=pos.data_ptr(),
                seg_ptr=seg.data_ptr())
    torch.cuda.synchronize()
    fit_ms, fit_wall, packed_ms, packed_wall = [], [], [], []
    for it in range(4):                                                  # the first round is the warm-up
        t = time.perf_counter()
        rows = mbpe.pack_fit(None, off, S, **common, **ptrs, cap_rows=n_fit, doc_row_ptr=d_row.data_ptr(),
                             doc_col_ptr=d_col.data_ptr())
        wall = (time.perf_counter() - t) * 1e3
        assert rows == n_fit
        if it:
            fit_ms.append(mbpe.pack_kernel_ms())
            fit_wall.append(wall)
        else:                                                            # what was written: every token's cell, once
            used = int((seg[:n_fit * S] != 0).sum())
            assert used == n_tok and int(pos[:n_fit * S].max()) == int(lens.max()) - 1, (used, n_tok)
            assert torch.equal(ln[:n_fit].cpu(), torch.from_numpy(plan["lengths"].view(np.int32)))
            assert np.array_equal(d_row.cpu().numpy().view(np.uint64), plan["doc_row"])
        t = time.perf_counter()
        rows = mbpe.pack_tokens_aux(None, off, S, layout="packed", **common, **ptrs, cap_rows=n_packed)
        wall = (time.perf_counter() - t) * 1e3
        assert rows == n_packed
        if it:
            packed_ms.append(mbpe.pack_kernel_ms())
            packed_wall.append(wall)
    per = lambda ms, rows: sorted(ms)[len(ms) // 2] * 1e9 / (rows * S)
    print("k_pack_fit ms", med(fit_ms), "cells", n_fit * S, "ps per cell %.3f" % per(fit_ms, n_fit))
    print("k_pack_aux PACKED ms", med(packed_ms), "cells", n_packed * S, "ps per cell %.3f" % per(packed_ms, n_packed))
    print("wall ms: pack_fit", med(fit_wall), "pack_tokens_aux PACKED", med(packed_wall))
    only = []
    for it in range(4):
        mbpe.pack_fit(None, off, S, **common, out_ptr=ids.data_ptr(), len_ptr=ln.data_ptr(), cap_rows=n_fit)
        if it:
            only.append(mbpe.pack_kernel_ms())
    print("k_pack_fit, ids and lengths only, ms", med(only))
    if which == "short":
        d_off = torch.from_numpy(off.view(np.int64)).to(dev)
        torch.cuda.synchronize()
        ts = []
        for _ in range(4):
            t = time.perf_counter()
            d_off.cpu()
            ts.append((time.perf_counter() - t) * 1e3)
        print("offsets, device to host, ms", med(ts[1:]), "bytes", off.nbytes)


def step_existing(label):
    import numpy as np
    import torch
    import mbpe
    dev = torch.device("cuda", 0)
    lens = np.random.default_rng(5).integers(1, 1025, 250000)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    n_tok = int(off[-1])
    d_tok = (torch.arange(n_tok, dtype=torch.int32, device=dev) % 60000) + 10
    common = dict(tokens_ptr=d_tok.data_ptr(), n_tokens=n_tok, token_bits=32)
    print(label, mbpe.lib().mbpe_version().decode())

    def run(name, fn, n_rows, S):
        ids, lab, pos, seg = (torch.empty(n_rows * S, dtype=torch.int32, device=dev) for _ in range(4))
        ln = torch.empty(n_rows, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        ms = []
        for it in range(6):
            rows = fn(dict(out_ptr=ids.data_ptr(), len_ptr=ln.data_ptr(), labels_ptr=lab.data_ptr(),
                           pos_ptr=pos.data_ptr(), seg_ptr=seg.data_ptr(), cap_rows=n_rows))
            assert rows == n_rows
            if it:
                ms.append(mbpe.pack_kernel_ms())
        print(label, name, "rows", n_rows, "seq_len", S, "ms", med(ms), flush=True)

    run("PADDED", lambda p: mbpe.pack_tokens_aux(None, off, 1024, layout="padded", **common, **p), len(lens), 1024)
    run("PACKED", lambda p: mbpe.pack_tokens_aux(None, off, 2048, layout="packed", **common, **p), -(-n_tok // 2048), 2048)
    W = np.where(lens <= 512, 1, 1 + -((512 - lens) // 384))
    run("windows", lambda p: mbpe.pack_windows(None, off, 512, 128, **common, **p), int(W.sum()), 512)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", help="a checkout of the parent commit whose libmbpe.so is built")
    ap.add_argument("--step", help=argparse.SUPPRESS)
    ap.add_argument("--root", default=ROOT, help=argparse.SUPPRESS)
    ap.add_argument("--label", default="tree", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        sys.path.insert(0, os.path.join(args.root, "minbpe-cc_amd", "python"))
        return step_existing(args.label) if args.step == "existing" else step_fit(args.step)
    steps = [("short", ROOT, "tree"), ("long", ROOT, "tree")]
    if args.parent_root:
        steps += [("existing", ROOT, "tree"), ("existing", args.parent_root, "parent")] * 2
    for step, root, label in steps:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--root", root, "--label", label]
        rc = subprocess.run(cmd, timeout=LIMIT).returncode
        if rc != 0:
            sys.exit("step %s (%s) ended with %d: nothing more is started" % (step, label, rc))


if __name__ == "__main__":
    main()
