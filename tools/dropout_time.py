"""BPE-dropout on the device timed (csrc/encode.hip, mbpe_encoder_set_dropout): shakespeare x --rep with the gpt4 split
and the golden gpt4 model, text and output on the device, kernel time of an Encoder call (mbpe_encoder_kernel_ms: HIP
events around widen, the passes and the finishing kernel; warm, median of --reps).

  plain     the default order and plain rank order of this build against another build of the library (--parent-root: a
            checkout of the parent commit with its libmbpe.so built).  The two builds are run alternately, --rounds
            processes each, parent first; the spread is what two runs of the parent itself differ by.  Condition: this
            build's median lies within the parent's median +- that spread, per order; same tokens.
  dropout   rank order with --dropout P against plain rank order of this build, by one process on one encoder: kernel
            ms, passes, tokens out and the tokens that entered every pass.  No limit is fixed.  The extra bytes as the
            kernels are written: 4 B read per lookup hit in k_enc_cand, 4 B read + 4 B written per kept token in the
            scatter, 4 B written per byte in widen.

Every step runs in a child process of its own under its own time limit; when one fails, nothing after it is started.

    python tools/dropout_time.py --parent-root <checkout of the parent commit> --json profiles/r19_dropout.json
"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SHAKESPEARE = os.path.join(ROOT, "tests", "golden", "data", "shakespeare.txt")
MODEL = os.path.join(ROOT, "tests", "golden", "shakespeare_gpt4_lexical_512.model")


def step_kernel(args):
    """One process of one build: greedy, rank and -- with --dropout -- rank with dropout, on one encoder."""
    sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), os.path.join(args.root, "minbpe-cc_amd", "python")]
    import numpy as np
    import torch
    import mbpe
    import oracle as O
    from encode_time import tiled
    if not torch.cuda.is_available():
        sys.exit("dropout_time.py needs a GPU: there is nothing to time without one")
    dev = torch.device("cuda", 0)
    sh = open(SHAKESPEARE, "rb").read()
    merges = O.parse_model(open(MODEL, "rb").read())[2]
    sh_off = mbpe.presplit(O.GPT4_SPLIT_PATTERN, sh)
    text = torch.from_numpy(np.frombuffer(sh, dtype=np.uint8).copy()).to(dev).repeat(args.rep)
    off = tiled(sh_off, len(sh), args.rep)
    out = torch.empty(text.numel() + 1, dtype=torch.int32, device=dev)
    modes = [("greedy", 0, None), ("rank", 1, None)]
    if args.dropout is not None:
        modes.append(("rank_dropout", 1, args.dropout))
    rows = []
    with mbpe.Encoder(merges) as enc:
        for name, rank, p in modes:
            enc.set_option("rank_order", rank)
            if args.dropout is not None:
                enc.set_dropout(p or 0.0, args.seed)

            def run():
                n = enc.encode_device(text.data_ptr(), text.numel(), off, out.data_ptr(), out.numel(), 32)
                return n, enc.kernel_ms()
            for _ in range(2):
                n_out, _ = run()
            ms = [run()[1] for _ in range(args.reps)]
            tokens = (out[:n_out] & 0x7FFFFFFF).cpu().numpy().astype("<u4")
            rows.append({"mode": name, "dropout": p, "text_bytes": text.numel(), "chunks": len(off) - 1, "tokens": n_out,
                         "passes": enc.n_passes, "pass_tokens": enc.pass_tokens(), "reps": args.reps,
                         "kernel_ms_median": statistics.median(ms), "kernel_ms_min": min(ms), "kernel_ms_max": max(ms),
                         "text_GBps": text.numel() / statistics.median(ms) / 1e6, "allocs": enc.alloc_count(),
                         "sha256": hashlib.sha256(tokens.tobytes()).hexdigest()})
    print(json.dumps({"lib": os.path.relpath(mbpe.LIB_PATH, ROOT), "version": mbpe.lib().mbpe_version().decode(),
                      "device": torch.cuda.get_device_name(0), "rows": rows}))


def child(limit, extra, log):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", "kernel"] + extra
    print("+", " ".join(cmd), flush=True)
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT)
    log.append({"args": [os.path.relpath(a, ROOT) if os.path.isabs(a) else a for a in extra], "exit": p.returncode,
                "stderr_tail": p.stderr[-2000:] if p.returncode else ""})
    if p.returncode != 0:
        print(p.stderr[-4000:], file=sys.stderr)
        return None
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["kernel"])
    ap.add_argument("--json")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--rep", type=int, default=1024, help="copies of shakespeare.txt")
    ap.add_argument("--dropout", type=float, default=None)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--limit", type=int, default=240, help="time limit of one child process in seconds")
    ap.add_argument("--parent-root", help="checkout of the parent commit with minbpe-cc_amd/libmbpe.so built")
    ap.add_argument("--root", default=ROOT)
    args = ap.parse_args()
    if args.step:
        return step_kernel(args)
    if not args.parent_root or not os.path.exists(os.path.join(args.parent_root, "minbpe-cc_amd", "libmbpe.so")):
        sys.exit("--parent-root must name a checkout of the parent commit with its libmbpe.so built")
    res, log = {}, []
    common = ["--reps", str(args.reps), "--rep", str(args.rep)]

    def done():
        res["log"] = log
        print(json.dumps(res))
        if args.json:
            with open(args.json, "w") as f:
                json.dump(res, f, indent=1)

    runs = {"parent": [], "this": []}
    for _ in range(args.rounds):                         # alternately: the parent's build, this build
        for who, root in (("parent", args.parent_root), ("this", ROOT)):
            extra = common + ["--root", root]
            if who == "this":
                extra += ["--dropout", str(0.1 if args.dropout is None else args.dropout), "--seed", str(args.seed)]
            r = child(args.limit, extra, log)
            if r is None:
                return done()
            runs[who].append(r)
    res["device"] = runs["this"][0]["device"]
    res["versions"] = {who: runs[who][0]["version"] for who in runs}
    plain = []
    for i, mode in enumerate(("greedy", "rank")):
        old = [r["rows"][i]["kernel_ms_median"] for r in runs["parent"]]
        new = [r["rows"][i]["kernel_ms_median"] for r in runs["this"]]
        spread = max(old) - min(old)
        same = len(set(r["rows"][i]["sha256"] for who in runs for r in runs[who])) == 1
        row = {"mode": mode, "parent_ms": old, "this_ms": new, "parent_spread_ms": spread, "same_tokens": same,
               "passes": runs["this"][0]["rows"][i]["passes"], "tokens": runs["this"][0]["rows"][i]["tokens"],
               "allocs": {who: runs[who][0]["rows"][i]["allocs"] for who in runs},
               "within_spread": same and abs(statistics.median(new) - statistics.median(old)) <= spread}
        plain.append(row)
    res["plain"] = plain
    res["dropout"] = [{k: r["rows"][i][k] for k in ("mode", "dropout", "tokens", "passes", "pass_tokens", "kernel_ms_median",
                                                    "kernel_ms_min", "kernel_ms_max", "text_GBps", "allocs")}
                      for r in runs["this"] for i in (1, 2)]
    done()


if __name__ == "__main__":
    main()
