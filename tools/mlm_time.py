"""Masked-LM batches on the device (csrc/mlm.hip, the label stream of csrc/pack.hip) timed.  Every step below runs in a
child process of its own under its own time limit; when one fails, nothing after it is started.

  stage     mbpe_mlm_tokens at rate 0.15 over 32-bit flagged tokens in device memory into device memory, token-level
            (mbpe_mlm_kernel_ms: k_mlm_apply) and whole-word (k_mlm_starts, k_mlm_scan, k_mlm_apply), alternating in
            every repetition with mbpe_fim_tokens at rate 0.5 (mbpe_fim_kernel_ms), mbpe_pack_tokens PACKED
            (mbpe_pack_kernel_ms: k_pack_stream) and a plain device-to-device copy of the tokens over the same buffers,
            on the two workloads of profiles/r28_fim.md: "short", 1,000,000 documents of 1 .. 1,024 tokens, and "long",
            1,000 documents of 600,000 tokens.
  packers   mbpe_pack_tokens_aux PACKED, mbpe_pack_windows and mbpe_pack_fit with labels, positions and segments in
            device memory on the "short" workload (mbpe_pack_kernel_ms), without and -- where the library has it --
            with a label stream.  --parent-root names a checkout of the parent commit with its library built: the step
            then runs against that library and its own Python package too, alternating with this one, twice each.

    python tools/mlm_time.py --json profiles/r29_mlm.json [--parent-root <parent checkout>]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

# (a child that measures the parent commit gets that checkout's package through MBPE_MLM_TIME_PKG)
sys.path[:0] = [os.environ.get("MBPE_MLM_TIME_PKG") or os.path.join(ROOT, "minbpe-cc_amd", "python")]


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "all": xs}


def workload(name, np):
    rng = np.random.default_rng(7)
    lens = rng.integers(1, 1025, size=1000000) if name == "short" else np.full(1000, 600000)
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)


def step_stage(args):
    import numpy as np
    import torch
    import mbpe
    dev = torch.device("cuda", 0)
    off = workload(args.workload, np)
    n, n_docs = int(off[-1]), len(off) - 1
    seq_len = 2048 if args.workload == "short" else 512
    ids = torch.arange(n, dtype=torch.int64, device=dev) % 50000
    ends = (ids * 2654435761 >> 7) % 3 == 0                      # words of 3 tokens on average
    tokens = (ids | (ends.to(torch.int64) << 31)).to(torch.int32)
    del ids, ends
    out = torch.empty(n + 3 * n_docs, dtype=torch.int32, device=dev)
    tgt = torch.empty(n, dtype=torch.int32, device=dev)
    n_rows = -(-n // seq_len)
    mat = torch.empty((n_rows, seq_len), dtype=torch.int32, device=dev)
    ln = torch.empty(n_rows, dtype=torch.int32, device=dev)
    specs = {"token": mbpe.mlm_spec(0.15, 50001, 50000, seed=1), "word": mbpe.mlm_spec(0.15, 50001, 50000, seed=1, whole_word=True)}
    fim = mbpe.fim_spec(0.5, 0.5, 60001, 60002, 60003, seed=1)
    src = dict(tokens_ptr=tokens.data_ptr(), n_tokens=n, token_bits=32)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    ms = {k: [] for k in ("token", "word", "fim", "pack", "copy")}
    for i in range(1 + args.reps):
        row = {}
        for k, s in specs.items():
            mbpe.mlm_tokens(None, off, s, out_ptr=out.data_ptr(), targets_ptr=tgt.data_ptr(), **src)
            row[k] = mbpe.mlm_kernel_ms()
        mbpe.fim_tokens(None, off, fim, out_ptr=out.data_ptr(), cap=out.numel(), **src)
        row["fim"] = mbpe.fim_kernel_ms()
        mbpe.pack_tokens(None, off, seq_len, layout="packed", out_ptr=mat.data_ptr(), len_ptr=ln.data_ptr(), cap_rows=n_rows, **src)
        row["pack"] = mbpe.pack_kernel_ms()
        e0.record()
        out[:n].copy_(tokens)
        e1.record()
        torch.cuda.synchronize()
        row["copy"] = e0.elapsed_time(e1)
        if i:
            for k, v in row.items():
                ms[k].append(v)
    selected = int((tgt != -1).sum())
    med = {k: statistics.median(v) for k, v in ms.items()}
    copy_GBps = 8 * n / med["copy"] / 1e6                        # 4 B read and 4 B written per token
    res = {"step": "stage", "workload": args.workload, "device": torch.cuda.get_device_name(0),
           "lib": mbpe.lib().mbpe_version().decode(), "documents": n_docs, "tokens": n, "selected_whole_word": selected,
           "kernel_ms": {k: spread(v) for k, v in ms.items()}, "copy_GBps": copy_GBps,
           "token_GBps": 12 * n / med["token"] / 1e6, "word_GBps": (16 * n + 24 * (n // 1024)) / med["word"] / 1e6,
           "ratio_token_to_pack": med["token"] / med["pack"], "ratio_word_to_pack": med["word"] / med["pack"],
           "ratio_token_to_fim": med["token"] / med["fim"], "ratio_word_to_fim": med["word"] / med["fim"]}
    res["token_share_of_copy"] = res["token_GBps"] / copy_GBps
    res["word_share_of_copy"] = res["word_GBps"] / copy_GBps
    print(json.dumps(res))


def step_packers(args):
    import numpy as np
    import torch
    import mbpe
    dev = torch.device("cuda", 0)
    off = workload("short", np)
    n = int(off[-1])
    tokens = (torch.arange(n, dtype=torch.int64, device=dev) % 50000).to(torch.int32)
    tgt = torch.where(torch.arange(n, device=dev) % 7 == 0, tokens, torch.full_like(tokens, -1))
    src = dict(tokens_ptr=tokens.data_ptr(), n_tokens=n, token_bits=32)
    has_labels = hasattr(mbpe, "mlm_tokens")
    L = np.diff(off).astype(np.int64)
    win_rows = int(np.where(L <= 256, 1, 1 + -((256 - L) // (256 - 64))).sum())
    calls = {
        "aux packed": (mbpe.pack_tokens_aux, dict(seq_len=2048, layout="packed"), -(-n // 2048)),
        "windows": (mbpe.pack_windows, dict(seq_len=256, stride=64), win_rows),
        "fit": (mbpe.pack_fit, dict(seq_len=2048), int(mbpe.pack_fit_plan(off, 2048)["n_rows"])),
    }
    res = {"step": "packers", "device": torch.cuda.get_device_name(0), "lib": mbpe.lib().mbpe_version().decode(),
           "tokens": n, "calls": {}}
    for name, (fn, kw, n_rows) in calls.items():
        bufs = [torch.empty((n_rows, kw["seq_len"]), dtype=torch.int32, device=dev) for _ in range(4)]
        ln = torch.empty(n_rows, dtype=torch.int32, device=dev)
        out = dict(out_ptr=bufs[0].data_ptr(), len_ptr=ln.data_ptr(), cap_rows=n_rows, labels_ptr=bufs[1].data_ptr(),
                   pos_ptr=bufs[2].data_ptr(), seg_ptr=bufs[3].data_ptr())
        torch.cuda.synchronize()
        plain, labelled = [], []
        for i in range(1 + args.reps):
            assert fn(None, off, **kw, **src, **out) == n_rows
            a = mbpe.pack_kernel_ms()
            if has_labels:
                assert fn(None, off, label_tokens=tgt.data_ptr(), **kw, **src, **out) == n_rows
                b = mbpe.pack_kernel_ms()
            if i:
                plain.append(a)
                if has_labels:
                    labelled.append(b)
        res["calls"][name] = {"rows": n_rows, "seq_len": kw["seq_len"], "kernel_ms": spread(plain)}
        if has_labels:
            res["calls"][name]["kernel_ms_label_stream"] = spread(labelled)
        del bufs
        torch.cuda.empty_cache()
    print(json.dumps(res))


STEPS = {"stage": step_stage, "packers": step_packers}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--step", choices=sorted(STEPS))
    ap.add_argument("--workload", choices=["short", "long"], default="short")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-root", help="a checkout of the parent commit, built: the packers step runs against it too")
    ap.add_argument("--json")
    ap.add_argument("--timeout", type=int, default=240)
    args = ap.parse_args()
    if args.step:
        STEPS[args.step](args)
        return 0
    plan = [("stage", ["--workload", "short"], None), ("stage", ["--workload", "long"], None), ("packers", [], None)]
    if args.parent_root:
        parent = os.path.join(os.path.abspath(args.parent_root), "minbpe-cc_amd")
        plan += [("packers", [], parent), ("packers", [], None), ("packers", [], parent)]
    results = []
    for step, extra, lib in plan:
        env = dict(os.environ)
        if lib:
            env.update(MBPE_LIB=os.path.join(lib, "libmbpe.so"), MBPE_MLM_TIME_PKG=os.path.join(lib, "python"))
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--reps", str(args.reps)]
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
