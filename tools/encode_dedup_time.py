#!/usr/bin/env python3
"""Timing of the encoder's "dedup" route against the default routes (profiles/r21_encode_dedup.md).

The texts of r20 (tests/golden/data/<name>.txt repeated to about --gbytes GB, gpt4 pattern, split on the device, the
merges of the committed 512-entry model of that text):

  endmask   Encoder.encode_endmask into device memory, kernel ms (mbpe_encoder_kernel_ms), warm, median of --reps calls
            with min and max; both orders; dedup off and -- on this build -- on, there split into dedup (a Deduper with
            "map" by itself on the same text and mask), expansion (dedup_stats) and the rest: passes + finishing kernel.
            The expansion's bytes per second against what it has to move: unique_of read twice and the output written
  tokenizer Tokenizer.encode(device=0, device_split=True) end to end on the host clock, both orders; this build with
            dedup=True, the parent build as it is
  losing    1 GiB of SplitMix64 bytes cut every 8 bytes (nearly every chunk distinct) and as one chunk: kernel ms with
            dedup off and on, this build
  default   dedup off, both orders, on the first text: the parent build and this build alternately (twice each) in one
            call; the bar for "did not move" is the parent's own spread between its two runs
  --parent-endmask  (a parent that has the "dedup" route: profiles/r22_encode_host.md) the endmask job alternates the
            builds in the same way
  bench     bench.py --gpus 1 --steps 3 --warmup 1 of both builds alternately (twice each)

Every (build, job) is one child process; the builds alternate.  A run needs a GPU and torch (the output buffers):

    python tools/encode_dedup_time.py --parent-root <checkout of the parent commit, built> --json profiles/r21_encode_dedup.json
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "data")
GOLDEN = os.path.join(ROOT, "tests", "golden")
MODELS = {"shakespeare": "shakespeare_gpt4_lexical_512", "taylorswift": "taylorswift_gpt4_lexical_512"}


def _text(name, gbytes):
    with open(os.path.join(DATA, name + ".txt"), "rb") as f:
        one = f.read()
    copies = max(1, int(round(gbytes * 1e9 / len(one))))
    return one * copies, copies


def _med(ms):
    ms = sorted(ms)
    return {"median": ms[len(ms) // 2], "min": ms[0], "max": ms[-1]}


def worker(args):
    pkg = args.pkg_root or ROOT                 # the binding and the library of that checkout go together
    sys.path.insert(0, os.path.join(pkg, "minbpe-cc_amd", "python"))
    sys.path.insert(0, os.path.join(pkg, "oracle"))
    import numpy as np
    import torch
    import mbpe
    import oracle as O
    pattern = O.GPT4_SPLIT_PATTERN
    dev = torch.device("cuda", 0)
    has_dedup = "mbpe_encoder_dedup_stats" in mbpe.EXPORTS
    with open(os.path.join(GOLDEN, MODELS.get(args.text, MODELS["shakespeare"]) + ".model"), "rb") as f:
        merges = O.parse_model(f.read())[2]
    out = {"job": args.job, "text": args.text, "rows": []}

    def emit(row):
        out["rows"].append(row)
        print("#", json.dumps(row), flush=True)

    def timed(enc, call):
        ms = []
        for _ in range(args.reps + 1):
            n = call()
            ms.append(enc.kernel_ms())
        return n, _med(ms[1:])

    def endmask_rows(t_ptr, n_bytes, m_ptr, dedups, label):
        buf = torch.empty(n_bytes, dtype=torch.int32, device=dev)
        dd_ms = None
        if has_dedup and 1 in dedups:
            with mbpe.Deduper(0) as dd:
                dd.set_option("map", 1)
                ms = []
                for _ in range(args.reps + 1):
                    dd.chunks_endmask(t_ptr, n_bytes, m_ptr)
                    ms.append(dd.kernel_ms())
                dd_ms = _med(ms[1:])
        for order in ("greedy", "rank"):
            for dedup in dedups:
                kw = {"dedup": True} if dedup else {}
                with mbpe.Encoder(merges, rank_order=order == "rank", **kw) as enc:
                    n, ms = timed(enc, lambda: enc.encode_endmask(t_ptr, n_bytes, m_ptr, out_ptr=buf.data_ptr(), cap=n_bytes)[0])
                    row = {"case": label, "order": order, "dedup": bool(dedup), "bytes": n_bytes, "tokens": n,
                           "passes": enc.n_passes, "kernel_ms": ms, "measured": True}
                    if dedup:
                        st = enc.dedup_stats()
                        moved = 8 * st["n_chunks"] + 4 * n
                        row.update(st, dedup_ms=dd_ms, passes_finish_ms=ms["median"] - st["expand_ms"] - dd_ms["median"],
                                   expand_bytes=moved, expand_gb_per_s=moved / st["expand_ms"] / 1e6)
                    emit(row)

    if args.job in ("endmask", "default"):
        data, copies = _text(args.text, args.gbytes)
        out["copies"], out["bytes"] = copies, len(data)
        with mbpe.Splitter(pattern) as sp:
            out["chunks"] = sp.split(data, offsets=False)
            m_ptr, _, t_ptr = sp.endmask()
            endmask_rows(t_ptr, len(data), m_ptr, (0, 1) if has_dedup and args.job == "endmask" else (0,), args.text)
    elif args.job == "tokenizer":
        data, copies = _text(args.text, args.gbytes)
        tok = mbpe.Tokenizer(pattern)
        tok.set_merges(merges)
        tok.encode(data[:1 << 20], device=0, device_split=True)               # code objects loaded, device warm
        for order in ("greedy", "rank"):
            kw = {"dedup": True} if has_dedup else {}
            secs = []
            for _ in range(max(args.reps // 2, 2)):
                t0 = time.perf_counter()
                got = tok.encode(data, device=0, device_split=True, order=order, **kw)
                secs.append(time.perf_counter() - t0)
            emit({"case": "Tokenizer.encode " + args.text, "order": order, "dedup": bool(kw), "bytes": len(data),
                  "tokens": len(got), "seconds": _med(secs), "measured": True})
        tok.close()
    elif args.job == "losing":
        n = 1 << 30
        data = O.splitmix64_bytes(21, n)
        text = torch.from_numpy(data).to(dev)
        mask_bytes = (n + 15) // 16 * 2 + 16
        for label, every in (("splitmix 1 GiB cut every 8 bytes", 8), ("splitmix 1 GiB as one chunk", 0)):
            mask = torch.zeros(mask_bytes, dtype=torch.uint8, device=dev)
            if every:
                mask[:n // 8] = 0x80                                         # bit 7 of every byte: text bytes 7, 15, ..
            else:
                mask[(n - 1) >> 3] = 1 << ((n - 1) & 7)
            torch.cuda.synchronize()
            endmask_rows(text.data_ptr(), n, mask.data_ptr(), (0, 1), label)
    print(json.dumps(out), flush=True)


def child(pkg_root, job, text, args):
    env = dict(os.environ)
    env.pop("MBPE_LIB", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--pkg-root", pkg_root, "--job", job, "--text", text,
           "--gbytes", str(args.gbytes), "--reps", str(args.reps)]
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


def bench(root):
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1"],
                       cwd=root, capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit("bench.py failed in %s: %s" % (root, r.stderr[-2000:]))
    row = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    print("#", json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--job", default="endmask")
    ap.add_argument("--jobs", default="endmask,tokenizer,losing,default,bench")
    ap.add_argument("--text", default="shakespeare")
    ap.add_argument("--texts", default="shakespeare,taylorswift")
    ap.add_argument("--gbytes", type=float, default=1.14)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pkg-root", help="(worker) the checkout whose binding and library are timed")
    ap.add_argument("--parent-root", help="checkout of the parent commit with minbpe-cc_amd/libmbpe.so built")
    ap.add_argument("--parent-endmask", action="store_true", help="run the endmask job on the parent build too, alternately")
    ap.add_argument("--json")
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    parent_lib = os.path.join(args.parent_root or "", "minbpe-cc_amd", "libmbpe.so")
    if not args.parent_root or not os.path.exists(parent_lib):
        sys.exit("--parent-root must name a checkout of the parent commit with its libmbpe.so built")
    parent = os.path.abspath(args.parent_root)
    jobs = args.jobs.split(",")
    texts = args.texts.split(",")
    result = {"gbytes": args.gbytes, "reps": args.reps, "runs": []}

    def run(build, job, text):
        result["runs"].append({"build": build, **child(parent if build == "parent" else ROOT, job, text, args)})
        if args.json:                           # kept as it grows: a run that is cut short leaves what it measured
            with open(args.json, "w") as f:
                json.dump(result, f, indent=1)

    for text in texts:
        if "endmask" in jobs:
            for build in ("parent", "this", "parent", "this") if args.parent_endmask else ("this",):
                run(build, "endmask", text)
        if "tokenizer" in jobs:
            run("parent", "tokenizer", text)
            run("this", "tokenizer", text)
    if "losing" in jobs:
        run("this", "losing", "shakespeare")
    if "default" in jobs:
        for build in ("parent", "this", "parent", "this"):
            run(build, "default", texts[0])
    if "bench" in jobs:
        for build in ("parent", "this", "parent", "this"):
            result["runs"].append({"build": build, "job": "bench", "rows": [bench(parent if build == "parent" else ROOT)]})
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
