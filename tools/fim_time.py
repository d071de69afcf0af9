"""Fill-in-the-middle on the device (csrc/fim.hip) timed.  Every step below runs in a child process of its own under
its own time limit; when one fails, nothing after it is started.

  stage     mbpe_fim_tokens at rate 0.5 / spm 0.5 over 32-bit tokens in device memory into device memory
            (mbpe_fim_kernel_ms: k_fim_plan, the scan, k_fim_offsets and k_fim_gather), alternating with
            mbpe_pack_tokens PACKED over the same tokens (mbpe_pack_kernel_ms: k_pack_stream), on the two workloads of
            profiles/r27_pack_fit.md: "short", 1,000,000 documents of 1 .. 1,024 tokens in rows of 2,048, and "long",
            1,000 documents of 600,000 tokens in rows of 512.  Both read and write every token once.
  encoder   the four encoder batch calls (PACKED, aux PACKED, windows, fit) with fill-in-the-middle off, matrices in
            device memory, over shakespeare x --rep with every line a document: mbpe_encoder_kernel_ms,
            mbpe_encoder_pack_ms and the wall clock of every repetition.  --parent-root names a checkout of the parent
            commit with its library built: the step then runs against that library and its own Python package too,
            alternating with this one, twice each.

    python tools/fim_time.py --json profiles/r28_fim.json [--parent-root <parent checkout>] [--skip-stage]
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
PRE, SUF, MID = 60001, 60002, 60003

# (a child that measures the parent commit gets that checkout's package through MBPE_FIM_TIME_PKG)
sys.path[:0] = [os.path.join(ROOT, "oracle"),
                os.environ.get("MBPE_FIM_TIME_PKG") or os.path.join(ROOT, "minbpe-cc_amd", "python")]


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "all": xs}


def step_stage(args):
    import numpy as np
    import torch
    import mbpe
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(7)
    if args.workload == "short":
        lens, seq_len = rng.integers(1, 1025, size=1000000), 2048
    else:
        lens, seq_len = np.full(1000, 600000), 512
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    n, n_docs = int(off[-1]), len(lens)
    tokens = (torch.arange(n, dtype=torch.int64, device=dev) % 50000).to(torch.int32)
    spec = mbpe.fim_spec(0.5, 0.5, PRE, SUF, MID, seed=1)
    new_off, mode, _ = mbpe.fim_plan(off, spec)
    n_new = int(new_off[-1])
    out = torch.empty(n_new, dtype=torch.int32, device=dev)
    n_rows = -(-n // seq_len)
    ids = torch.empty((n_rows, seq_len), dtype=torch.int32, device=dev)
    ln = torch.empty(n_rows, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    fim_ms, pack_ms, fim_wall = [], [], []
    for i in range(1 + args.reps):
        t = time.perf_counter()
        got, _ = mbpe.fim_tokens(None, off, spec, tokens_ptr=tokens.data_ptr(), n_tokens=n, token_bits=32,
                                 out_ptr=out.data_ptr(), cap=n_new)
        w = time.perf_counter() - t
        assert got == n_new
        rows = mbpe.pack_tokens(None, off, seq_len, layout="packed", tokens_ptr=tokens.data_ptr(), n_tokens=n, token_bits=32,
                                out_ptr=ids.data_ptr(), len_ptr=ln.data_ptr(), cap_rows=n_rows)
        assert rows == n_rows
        if i:
            fim_ms.append(mbpe.fim_kernel_ms()); pack_ms.append(mbpe.pack_kernel_ms()); fim_wall.append(w)
    # the untransformed documents are copies: a spot check that the kernel wrote what the plan says
    d = int(np.flatnonzero(mode == 0)[0])
    a, b = int(off[d]), int(off[d + 1])
    assert torch.equal(out[int(new_off[d]):int(new_off[d + 1])], tokens[a:b])
    f, p = statistics.median(fim_ms), statistics.median(pack_ms)
    fim_bytes = 4 * n + 4 * n_new + n_docs * (16 + 8 * 3 + 17 + 41)
    pack_bytes = 4 * n + 4 * n_rows * seq_len + 4 * n_rows + 8 * (n_docs + 1)
    print(json.dumps({
        "step": "stage", "workload": args.workload, "device": torch.cuda.get_device_name(0),
        "lib": mbpe.lib().mbpe_version().decode(), "documents": n_docs, "tokens": n, "tokens_after": n_new,
        "transformed": int((mode != 0).sum()), "seq_len": seq_len, "fim_kernel_ms": spread(fim_ms),
        "pack_stream_kernel_ms": spread(pack_ms), "fim_wall_s": spread(fim_wall), "ratio_fim_to_pack": f / p,
        "fim_bytes": fim_bytes, "pack_bytes": pack_bytes, "fim_GBps": fim_bytes / f / 1e6, "pack_GBps": pack_bytes / p / 1e6}))


def step_encoder(args):
    import numpy as np
    import torch
    import mbpe
    import oracle as O
    dev = torch.device("cuda", 0)
    sh = open(SHAKESPEARE, "rb").read()
    merges = O.parse_model(open(MODEL, "rb").read())[2]
    pattern = mbpe.split_pattern("gpt4")
    parts, first, at = [], [0], 0
    for x in sh.splitlines(keepends=True):                           # every line split on its own
        o = mbpe.presplit(pattern, x)
        parts.append(o[1:] + np.uint64(at))
        at += len(x)
        first.append(first[-1] + len(o) - 1)
    one_off, one_doc = np.concatenate([[0]] + parts).astype(np.uint64), np.array(first, dtype=np.uint64)
    rep = args.rep
    off = np.concatenate([[0]] + [one_off[1:] + np.uint64(r * len(sh)) for r in range(rep)]).astype(np.uint64)
    docs = np.concatenate([[0]] + [one_doc[1:] + np.uint64(r * (len(one_off) - 1)) for r in range(rep)]).astype(np.uint64)
    text = torch.from_numpy(np.frombuffer(sh, dtype=np.uint8).copy()).to(dev).repeat(rep)
    torch.cuda.synchronize()
    src = dict(text_ptr=text.data_ptr(), n_bytes=text.numel())
    res = {"step": "encoder", "device": torch.cuda.get_device_name(0), "lib": mbpe.lib().mbpe_version().decode(),
           "rep": rep, "text_bytes": text.numel(), "documents": len(docs) - 1, "calls": {}}
    with mbpe.Encoder(merges) as enc:
        calls = {
            "packed": (enc.encode_batch, dict(seq_len=2048, layout="packed"), 2048, False),
            "aux packed": (enc.encode_batch_aux, dict(seq_len=2048, layout="packed"), 2048, True),
            "windows": (enc.encode_batch_windows, dict(seq_len=64, stride=16), 64, True),
            "fit": (enc.encode_batch_fit, dict(seq_len=2048), 2048, True),
        }
        for name, (fn, kw, seq_len, aux) in calls.items():
            sized = fn(None, off, docs, **kw, **src)                  # host matrices once: the row count
            n_rows = len(sized["ids"] if isinstance(sized, dict) else sized[0])
            del sized
            d_ids = torch.empty((n_rows, seq_len), dtype=torch.int32, device=dev)
            d_len = torch.empty(n_rows, dtype=torch.int32, device=dev)
            out = dict(out_ptr=d_ids.data_ptr(), len_ptr=d_len.data_ptr(), cap_rows=n_rows)
            if aux:
                d_lab, d_pos, d_seg = (torch.empty((n_rows, seq_len), dtype=torch.int32, device=dev) for _ in range(3))
                out.update(labels_ptr=d_lab.data_ptr(), pos_ptr=d_pos.data_ptr(), seg_ptr=d_seg.data_ptr())
            torch.cuda.synchronize()
            total, pack, wall = [], [], []
            for i in range(1 + args.reps):
                t = time.perf_counter()
                got = fn(None, off, docs, **kw, **src, **out)
                w = time.perf_counter() - t
                assert got == n_rows
                if i:
                    total.append(enc.kernel_ms()); pack.append(enc.pack_ms()); wall.append(w)
            res["calls"][name] = {"rows": n_rows, "seq_len": seq_len, "tokens": enc.n_tokens, "kernel_ms": spread(total),
                                  "pack_ms": spread(pack), "wall_s": spread(wall)}
            torch.cuda.empty_cache()
    print(json.dumps(res))


STEPS = {"stage": step_stage, "encoder": step_encoder}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--step", choices=sorted(STEPS))
    ap.add_argument("--workload", choices=["short", "long"], default="short")
    ap.add_argument("--rep", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-root", help="a checkout of the parent commit, built: the encoder step runs against it too")
    ap.add_argument("--skip-stage", action="store_true", help="the encoder step alone")
    ap.add_argument("--json")
    ap.add_argument("--timeout", type=int, default=240)
    args = ap.parse_args()
    if args.step:
        STEPS[args.step](args)
        return 0
    plan = [] if args.skip_stage else [("stage", ["--workload", "short"], None), ("stage", ["--workload", "long"], None)]
    plan.append(("encoder", [], None))
    if args.parent_root:
        parent = os.path.join(os.path.abspath(args.parent_root), "minbpe-cc_amd")
        plan += [("encoder", [], parent), ("encoder", [], None), ("encoder", [], parent)]
    results = []
    for step, extra, lib in plan:
        env = dict(os.environ)
        if lib:
            env.update(MBPE_LIB=os.path.join(lib, "libmbpe.so"), MBPE_FIM_TIME_PKG=os.path.join(lib, "python"))
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--rep", str(args.rep), "--reps", str(args.reps)]
        try:
            r = subprocess.run(cmd + extra, capture_output=True, text=True, timeout=args.timeout, env=env)
        except subprocess.TimeoutExpired:
            print("step %s ran into its time limit" % step, file=sys.stderr)
            break
        if r.returncode != 0:
            print("step %s failed (%d):\n%s" % (step, r.returncode, r.stderr[-3000:]), file=sys.stderr)
            break
        row = json.loads(r.stdout.strip().splitlines()[-1])
        row["which"] = "parent" if lib else "this"
        results.append(row)
        print(json.dumps(row))
        sys.stdout.flush()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)
    return 0 if len(results) == len(plan) else 1


if __name__ == "__main__":
    sys.exit(main())
