#!/usr/bin/env python3
"""Timing of the weighted 32-bit training loop with and without the stopping rules (profiles/r23_train_limits.md).

The workload of profiles/r20_dedup.md: tests/golden/data/shakespeare.txt repeated to about --gbytes GB, gpt4 pattern,
split and deduplicated on the device, the deduper's result loaded with Trainer.load_corpus_endmask_weighted, vocab
--vocab, both tie-breaks.  Per configuration: merges per second from mbpe_stats.ms_steps (device events around the
groups of merges), the merges made and the longest token.

  off      limits off, on this build and on the parent commit's build (--parent-root: a checkout of the parent commit with
           its libmbpe.so built), --rounds times, alternating: parent, this, parent, this ...  The unlimited kernels are
           meant to be the parent's code, so the bar for "this" is the parent's own spread between its rounds.
  limited  this build only, for information: max_token_length 8, 16 and min_frequency 2

Every (build, round) is one child process; the text is split and deduplicated once per process.  A run needs a GPU:

    python tools/train_limits_time.py --parent-root <checkout of the parent commit> --json profiles/r23_train_limits.json
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "data")


def worker(args):
    pkg = args.pkg_root or ROOT                 # the binding and the library of that checkout go together
    sys.path.insert(0, os.path.join(pkg, "minbpe-cc_amd", "python"))
    sys.path.insert(0, os.path.join(pkg, "oracle"))
    import mbpe
    import oracle as O
    pattern = O.GPT4_SPLIT_PATTERN
    with open(os.path.join(DATA, args.text + ".txt"), "rb") as f:
        one = f.read()
    copies = max(1, int(round(args.gbytes * 1e9 / len(one))))
    data = one * copies
    out = {"text": args.text, "copies": copies, "bytes": len(data), "rows": []}
    mbpe.Tokenizer(pattern).train(one, 300, device_split=True)             # code objects loaded, device warm
    with mbpe.Splitter(pattern) as sp, mbpe.Deduper(0) as dd:
        sp.split(data, offsets=False)
        m_ptr, _, t_ptr = sp.endmask()
        nu, nb = dd.chunks_endmask(t_ptr, len(data), m_ptr)
        t_u, m_u, w_u, _ = dd.result()
        out.update(n_unique=nu, n_unique_bytes=nb)
        for job in args.jobs.split(";"):
            cr, L, f = (int(x) for x in job.split(":"))
            with mbpe.Trainer(0) as tr:
                tr.load_corpus_endmask_weighted(m_u, text_ptr=t_u, n_bytes=nb, weights_ptr=w_u, n_weights=nu)
                tr.set_option("conflict_resolution", cr)
                if L or f:                      # (the parent's build does not know the options)
                    tr.set_option("max_token_length", L)
                    tr.set_option("min_frequency", f)
                t0 = time.perf_counter()
                tr.train_begin(args.vocab)
                tr.train_steps(args.vocab - 256)
                wall = time.perf_counter() - t0
                m, c = tr.train_result()
                st = tr.stats()
            length = [1] * 256
            for a, b in m.tolist():
                length.append(length[a] + length[b])
            row = {"conflict_resolution": "lexical" if cr else "first", "max_token_length": L, "min_frequency": f,
                   "merges": len(m), "longest_token": max(length), "last_count": int(c[-1]) if len(c) else None,
                   "ms_begin": st["ms_begin"], "ms_steps": st["ms_steps"], "wall_s": wall,
                   "merges_per_s_device": len(m) / (st["ms_steps"] / 1e3) if st["ms_steps"] else None,
                   "merges_sha": hashlib.sha256(m.tobytes()).hexdigest()[:16]}
            out["rows"].append(row)
            print("#", json.dumps(row), flush=True)
    print(json.dumps(out), flush=True)


def child(pkg_root, jobs, args):
    env = dict(os.environ)
    env.pop("MBPE_LIB", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--pkg-root", pkg_root, "--text", args.text, "--jobs",
           ";".join(jobs), "--gbytes", str(args.gbytes), "--vocab", str(args.vocab)]
    proc = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, text=True)
    last = ""
    for line in proc.stdout:                    # rows are shown as they come
        if line.startswith("#"):
            print(line.rstrip(), flush=True)
        elif line.strip():
            last = line
    if proc.wait() != 0:
        sys.exit("worker failed (%d): %s" % (proc.returncode, last[-2000:]))
    return json.loads(last)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--text", default="shakespeare")
    ap.add_argument("--jobs", default="")
    ap.add_argument("--gbytes", type=float, default=1.14)
    ap.add_argument("--vocab", type=int, default=10000)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--pkg-root", help="(worker) the checkout whose binding and library are timed")
    ap.add_argument("--parent-root", help="checkout of the parent commit with minbpe-cc_amd/libmbpe.so built")
    ap.add_argument("--json")
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    parent_lib = os.path.join(args.parent_root or "", "minbpe-cc_amd", "libmbpe.so")
    if not args.parent_root or not os.path.exists(parent_lib):
        sys.exit("--parent-root must name a checkout of the parent commit with its libmbpe.so built")
    off = ["1:0:0", "0:0:0"]
    limited = ["%d:%d:%d" % (cr, L, f) for cr in (1, 0) for L, f in ((8, 0), (16, 0), (0, 2))]
    result = {"gbytes": args.gbytes, "vocab": args.vocab, "runs": []}
    for r in range(args.rounds):
        result["runs"].append({"build": "parent", "round": r, **child(os.path.abspath(args.parent_root), off, args)})
        result["runs"].append({"build": "this", "round": r,
                               **child(ROOT, off + (limited if r == args.rounds - 1 else []), args)})
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
