#!/usr/bin/env python3
"""Timing of the word count across pieces and of trainings on a corpus fed in pieces (profiles/r22_wordcount.md).

Text: tests/golden/data/shakespeare.txt repeated to about --gbytes GB, gpt4 pattern, split on the device.

  count    kernel time of accumulating the text as 1, 8 and 64 pieces (sum of mbpe_wordcount_kernel_ms over the pieces: the
           owned deduper's kernels and the fold's), warm, median of --reps rounds, against Deduper.chunks_endmask on the
           whole text in the same process; device memory in use once every piece has been added (the buffers are kept)
  train    Tokenizer.train_from_iterator(device_split=True) over 8 pieces end to end (host clock), `first`, at the
           --vocabs, against Tokenizer.train(dedup=True) on the whole text; peak device memory of both, sampled every
           2 ms from a second thread while the call runs (hipMemGetInfo through torch)
  worst    256 MiB of SplitMix64 bytes cut every 8 bytes, in 4 pieces: every chunk is new and the append carries the bytes

--parent-root (optional): a checkout of the parent commit with its libmbpe.so built; its Deduper and its
Tokenizer.train(dedup=True) are timed in a child process of their own (the kinds "dedup" and "train-whole").

    python tools/wordcount_time.py --json profiles/r22_wordcount.json [--parent-root DIR]
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "data")


def _cut(text, n_pieces):
    """n_pieces pieces, cut where a letter or digit is followed by whitespace (a chunk boundary under gpt2 / gpt4)."""
    n, at = len(text), [0]
    for k in range(1, n_pieces):
        i = max(k * n // n_pieces, at[-1], 1)
        while i < n and not (chr(text[i - 1]).isascii() and chr(text[i - 1]).isalnum() and text[i] in b" \t\r\n"):
            i += 1
        at.append(i)
    at.append(n)
    view = memoryview(text)
    return [view[at[k]:at[k + 1]] for k in range(n_pieces)]


class PeakMemory:
    """Device memory in use (total - free), sampled from a second thread; .peak - .before = what the call added."""

    def __init__(self, torch):
        self.torch = torch
        self.before = self.peak = self._used()
        self._stop = threading.Event()
        self._thread = threading.Thread(target=self._run, daemon=True)

    def _used(self):
        free, total = self.torch.cuda.mem_get_info()
        return total - free

    def _run(self):
        while not self._stop.is_set():
            self.peak = max(self.peak, self._used())
            time.sleep(0.002)

    def __enter__(self):
        self._thread.start()
        return self

    def __exit__(self, *a):
        self._stop.set()
        self._thread.join()


def _sha(merges):
    return hashlib.sha256(merges.tobytes()).hexdigest()[:16]


def worker(args):
    pkg = args.pkg_root or ROOT
    sys.path.insert(0, os.path.join(pkg, "minbpe-cc_amd", "python"))
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import numpy as np
    import torch
    import mbpe
    import oracle as O
    pattern = O.GPT4_SPLIT_PATTERN
    with open(os.path.join(DATA, "shakespeare.txt"), "rb") as f:
        small = f.read()
    copies = max(1, int(round(args.gbytes * 1e9 / len(small))))
    data = small * copies
    torch.cuda.set_device(0)
    mbpe.Tokenizer(pattern).train(small, 300, device_split=True)            # code objects loaded, device warm
    rows = []

    def emit(row):
        rows.append(row)
        print("#", json.dumps(row), flush=True)

    def med(xs):
        xs = sorted(xs)
        return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}

    kinds = args.kinds.split(",")
    if "dedup" in kinds:
        with mbpe.Splitter(pattern) as sp, mbpe.Deduper(0) as dd:
            n_chunks = sp.split(data, offsets=False)
            m_ptr, _, t_ptr = sp.endmask()
            ms = []
            for _ in range(args.reps + 1):
                nu, nb = dd.chunks_endmask(t_ptr, len(data), m_ptr)
                ms.append(dd.kernel_ms())
            emit({"kind": "dedup", "bytes": len(data), "n_chunks": n_chunks, "n_unique": nu, "n_unique_bytes": nb,
                  "kernel_ms": med(ms[1:]), "split_kernel_ms": sp.kernel_ms()})
    if "count" in kinds:
        for n_pieces in (1, 8, 64):
            pieces = _cut(data, n_pieces)
            base = torch.cuda.mem_get_info()
            with mbpe.Splitter(pattern) as sp, mbpe.WordCount(0) as wc:
                totals, n_chunks = [], 0
                for rnd in range(args.reps + 1):
                    wc.reset()
                    total = 0.0
                    for p in pieces:
                        n = sp.split(np.frombuffer(p, dtype=np.uint8), offsets=False)
                        n_chunks += n if rnd == 0 else 0
                        m_ptr, _, t_ptr = sp.endmask()
                        wc.add_endmask(t_ptr, len(p), m_ptr)
                        total += wc.kernel_ms()
                    totals.append(total)
                used = base[0] - torch.cuda.mem_get_info()[0]
                st = wc.stats()
                emit({"kind": "count", "pieces": n_pieces, "largest_piece_bytes": max(len(p) for p in pieces),
                      "n_chunks": n_chunks, "kernel_ms": med(totals[1:]), "stats": st,
                      "device_bytes_splitter_and_wordcount": used, "allocations": wc.alloc_count()})
    if "train" in kinds or "train-whole" in kinds:
        for vocab in [int(v) for v in args.vocabs.split(",")]:
            if "train" in kinds:
                pieces = _cut(data, 8)
                tok = mbpe.Tokenizer(pattern)
                with PeakMemory(torch) as pm:
                    t0 = time.perf_counter()
                    tok.train_from_iterator((np.frombuffer(p, dtype=np.uint8) for p in pieces), vocab, conflict_resolution=0,
                                            device_split=True)
                    secs = time.perf_counter() - t0
                m = np.asarray(tok.merges(), dtype=np.uint32)
                emit({"kind": "train-pieces", "pieces": 8, "vocab": vocab, "seconds": secs, "merges": len(m),
                      "merges_sha": _sha(m), "peak_device_bytes": pm.peak - pm.before})
                tok.close()
            tok = mbpe.Tokenizer(pattern)
            with PeakMemory(torch) as pm:
                t0 = time.perf_counter()
                tok.train(data, vocab, conflict_resolution=0, device_split=True, dedup=True)
                secs = time.perf_counter() - t0
            m = np.asarray(tok.merges(), dtype=np.uint32)
            emit({"kind": "train-whole-dedup", "vocab": vocab, "seconds": secs, "merges": len(m), "merges_sha": _sha(m),
                  "peak_device_bytes": pm.peak - pm.before})
            tok.close()
    if "worst" in kinds:
        n = 256 << 20
        rnd = np.asarray(O.splitmix64_bytes(42, n), dtype=np.uint8)
        per = n // 4
        off = np.arange(0, per + 1, 8, dtype=np.uint64)
        with mbpe.WordCount(0) as wc, mbpe.Deduper(0) as dd:
            per_piece = []
            for k in range(4):
                wc.add(rnd[k * per:(k + 1) * per], off)
                per_piece.append(wc.kernel_ms())
            dd.chunks(rnd[:per], off)
            emit({"kind": "worst", "bytes": n, "pieces": 4, "kernel_ms_per_piece": per_piece, "stats": wc.stats(),
                  "dedup_alone_first_piece_ms": dd.kernel_ms()})
    print(json.dumps({"copies": copies, "bytes": len(data), "rows": rows}), flush=True)


def child(pkg_root, kinds, args):
    env = dict(os.environ)
    env.pop("MBPE_LIB", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--pkg-root", pkg_root, "--kinds", kinds,
           "--gbytes", str(args.gbytes), "--reps", str(args.reps), "--vocabs", args.vocabs]
    proc = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, text=True)
    last = ""
    for line in proc.stdout:
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
    ap.add_argument("--kinds", default="dedup,count,train,worst")
    ap.add_argument("--gbytes", type=float, default=1.14)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--vocabs", default="512,10000")
    ap.add_argument("--pkg-root")
    ap.add_argument("--parent-root")
    ap.add_argument("--json")
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    result = {"gbytes": args.gbytes, "runs": []}
    if args.parent_root:
        result["runs"].append({"build": "parent", **child(os.path.abspath(args.parent_root), "dedup,train-whole", args)})
    result["runs"].append({"build": "this", **child(ROOT, args.kinds, args)})
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
