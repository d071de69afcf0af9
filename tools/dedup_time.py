#!/usr/bin/env python3
"""Timing of the chunk deduplication and of trainings on unique chunks with counts (profiles/r20_dedup.md).

For every text (tests/golden/data/<name>.txt repeated to about --gbytes GB, gpt4 pattern, split on the device):

  dedup    kernel time of Deduper.chunks_endmask on the splitter's text and mask (mbpe_dedup_kernel_ms: HIP events around
           the kernels), warm, median of --reps calls; chunks, unique chunks, unique bytes; GB/s of text
  loop     the weighted 32-bit loop by itself: the deduper's result into Trainer.load_corpus_endmask_weighted, then
           merges per second from mbpe_stats.ms_steps (device events around the groups of merges), both tie-breaks
  train    Tokenizer.train(device_split=True) end to end (host clock around the call, which ends synchronised), both
           tie-breaks, at the --vocabs; with dedup=True on this build, without it on the parent commit's build
           (--parent-root: a checkout of the parent commit with its libmbpe.so built)
  capped   a configuration that would run for minutes without dedup is not run to its end: a Trainer on the same
           corpus steps in groups until --cap-seconds have passed, and the merges made and the time per merge of the
           latest group are reported

Every (text, build) pair is one child process, so that the text is built once; the builds alternate.  A run needs a GPU:

    python tools/dedup_time.py --parent-root <checkout of the parent commit> --json profiles/r20_dedup.json
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


def _text(name, gbytes):
    with open(os.path.join(DATA, name + ".txt"), "rb") as f:
        one = f.read()
    copies = max(1, int(round(gbytes * 1e9 / len(one))))
    return one * copies, copies


def _sha(merges):
    return hashlib.sha256(merges.tobytes()).hexdigest()[:16]


def worker(args):
    pkg = args.pkg_root or ROOT                 # the binding and the library of that checkout go together
    sys.path.insert(0, os.path.join(pkg, "minbpe-cc_amd", "python"))
    sys.path.insert(0, os.path.join(pkg, "oracle"))
    import numpy as np
    import mbpe
    import oracle as O
    pattern = O.GPT4_SPLIT_PATTERN
    data, copies = _text(args.text, args.gbytes)
    out = {"text": args.text, "copies": copies, "bytes": len(data), "rows": []}
    with open(os.path.join(DATA, args.text + ".txt"), "rb") as f:
        small = f.read()
    mbpe.Tokenizer(pattern).train(small, 300, device_split=True)            # code objects loaded, device warm

    def emit(row):
        out["rows"].append(row)
        print("#", json.dumps(row), flush=True)

    for job in args.jobs.split(";"):
        kind, vocab, cr, dedup = job.split(":")
        vocab, cr, dedup = int(vocab), int(cr), int(dedup)
        row = {"kind": kind, "vocab": vocab, "conflict_resolution": "lexical" if cr else "first", "dedup": bool(dedup)}
        if kind == "dedup":
            with mbpe.Splitter(pattern) as sp, mbpe.Deduper(0) as dd:
                n_chunks = sp.split(data, offsets=False)
                m_ptr, _, t_ptr = sp.endmask()
                ms = []
                for _ in range(args.reps + 1):
                    nu, nb = dd.chunks_endmask(t_ptr, len(data), m_ptr)
                    ms.append(dd.kernel_ms())
                ms = sorted(ms[1:])
                med = ms[len(ms) // 2]
                row.update(split_kernel_ms=sp.kernel_ms(), n_chunks=n_chunks, n_unique=nu, n_unique_bytes=nb,
                           kernel_ms_median=med, kernel_ms_min=ms[0], kernel_ms_max=ms[-1],
                           text_gb_per_s=len(data) / med / 1e6, allocations=dd.alloc_count())
                emit(row)
                t_u, m_u, w_u, _ = dd.result()
                for cr2 in (1, 0):
                    with mbpe.Trainer(0) as tr:
                        tr.load_corpus_endmask_weighted(m_u, text_ptr=t_u, n_bytes=nb, weights_ptr=w_u, n_weights=nu)
                        tr.set_option("conflict_resolution", cr2)
                        t0 = time.perf_counter()
                        tr.train_begin(vocab)
                        tr.train_steps(vocab - 256)
                        wall = time.perf_counter() - t0
                        m, c = tr.train_result()
                        st = tr.stats()
                    emit({"kind": "loop", "vocab": vocab, "conflict_resolution": "lexical" if cr2 else "first",
                          "merges": len(m), "ms_begin": st["ms_begin"], "ms_steps": st["ms_steps"], "wall_s": wall,
                          "merges_per_s_device": len(m) / (st["ms_steps"] / 1e3), "merges_per_s_wall": len(m) / wall,
                          "stream_tokens_at_end": st["n_live"], "last_count": int(c[-1]), "merges_sha": _sha(m)})
        elif kind == "train":
            tok = mbpe.Tokenizer(pattern)
            t0 = time.perf_counter()
            tok.train(data, vocab, conflict_resolution=cr, device_split=True, **({"dedup": True} if dedup else {}))
            row["seconds"] = time.perf_counter() - t0
            m = np.asarray(tok.merges(), dtype=np.uint32)
            row.update(merges=len(m), merges_sha=_sha(m))
            tok.close()
            emit(row)
        elif kind == "capped":
            with mbpe.Splitter(pattern) as sp, mbpe.Trainer(0) as tr:
                sp.split(data, offsets=False)
                m_ptr, _, t_ptr = sp.endmask()
                tr.load_corpus_endmask(m_ptr, text_ptr=t_ptr, n_bytes=len(data), keep=sp)
                tr.set_option("conflict_resolution", cr)
                tr.set_option("first_wide", 1)
                t0 = time.perf_counter()
                tr.train_begin(vocab)
                begin_s = time.perf_counter() - t0
                # (lexical: large groups, so that the slot stream's batches are not cut short by the group's limit)
                done, group, last = 0, args.cap_group * (128 if cr else 1), 0.0
                while done < vocab - 256 and time.perf_counter() - t0 < args.cap_seconds:
                    t1 = time.perf_counter()
                    n = tr.train_steps(min(group, vocab - 256 - done))
                    last = (time.perf_counter() - t1) / max(n, 1)
                    done += n
                    if n == 0:
                        break
                row.update(begin_s=begin_s, merges_done=done, seconds=time.perf_counter() - t0, finished=done >= vocab - 256,
                           ms_per_merge_latest_group=last * 1e3, group=group)
            emit(row)
    print(json.dumps(out), flush=True)


def child(pkg_root, text, jobs, args):
    env = dict(os.environ)
    env.pop("MBPE_LIB", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--pkg-root", pkg_root, "--text", text, "--jobs", ";".join(jobs),
           "--gbytes", str(args.gbytes), "--reps", str(args.reps), "--cap-seconds", str(args.cap_seconds),
           "--cap-group", str(args.cap_group)]
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
    ap.add_argument("--texts", default="shakespeare,taylorswift")
    ap.add_argument("--jobs", default="")
    ap.add_argument("--gbytes", type=float, default=1.14)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--vocabs", default="512,10000,100000")
    ap.add_argument("--cap-seconds", type=float, default=30.0)
    ap.add_argument("--cap-group", type=int, default=16)
    ap.add_argument("--pkg-root", help="(worker) the checkout whose binding and library are timed")
    ap.add_argument("--parent-root", help="checkout of the parent commit with minbpe-cc_amd/libmbpe.so built")
    ap.add_argument("--json")
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    parent_lib = os.path.join(args.parent_root or "", "minbpe-cc_amd", "libmbpe.so")
    if not args.parent_root or not os.path.exists(parent_lib):
        sys.exit("--parent-root must name a checkout of the parent commit with its libmbpe.so built")
    vocabs = [int(v) for v in args.vocabs.split(",")]
    # without dedup, on the parent: what finishes in seconds runs to its end (the slot stream's lexical batches, and
    # 256 merges of `first`); one pass over the corpus per merge for thousands of merges is capped
    slot_limit = 65518
    this_jobs = ["dedup:10000:1:0"] + ["train:%d:%d:1" % (v, cr) for v in vocabs for cr in (1, 0)]
    parent_jobs = []
    for v in vocabs:
        for cr in (1, 0):
            whole = v <= 512 or (cr == 1 and v <= slot_limit)
            if cr == 0 and v > min(x for x in vocabs if x > 512):
                continue                        # (`first` pays the same pass per merge at every larger vocabulary)
            parent_jobs.append("%s:%d:%d:0" % ("train" if whole else "capped", v, cr))
    result = {"gbytes": args.gbytes, "runs": []}
    for text in args.texts.split(","):
        result["runs"].append({"build": "parent", **child(os.path.abspath(args.parent_root), text, parent_jobs, args)})
        result["runs"].append({"build": "this", **child(ROOT, text, this_jobs, args)})
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
