#!/usr/bin/env python3
"""Timing of merging word-count tables (profiles/r24_wordcount_merge.md), in the manner of tools/wordcount_time.py.

  merge    tests/golden/data/shakespeare.txt repeated to about --gbytes GB, gpt4 pattern, split on the device, cut into 8
           pieces; every piece is counted into a WordCount of its own (8 tables), then the 8 tables are merged into an
           empty object.  Kernel time (sum of mbpe_wordcount_kernel_ms over the 8 merges), warm, median of --reps rounds:
             by object   mbpe_wordcount_merge: the fold alone (rehash, lookup, two scans, append)
             by blob     mbpe_wordcount_merge_blob: the fold plus k_wc_distinct, the device part of the validation;
                         the difference of the two is that kernel's cost
           and the host clock around the 8 blob merges (host-side check of the blob, two uploads, the kernels, the
           readbacks) and around the 8 exports.  For comparison in the same process: adding the same 8 pieces to one
           object (deduper + fold), and the deduper alone on each piece; add - dedup is the fold share of an add.
  worst    256 MiB of SplitMix64 bytes cut every 8 bytes, every chunk new, counted as 4 tables of 64 MiB and merged; the
           same two ways, per table, against adding the 4 pieces to one object.

    python tools/wordcount_merge_time.py --json profiles/r24_wordcount_merge.json
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "data")
sys.path.insert(0, os.path.join(ROOT, "tools"))


def med(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}


def merge_rounds(mbpe, tables, blobs, reps):
    """-> kernel ms by object and by blob (sum over the tables, and per table of the last round), host seconds of the
    blob merges."""
    by_object, by_blob, blob_seconds, per_object, per_blob = [], [], [], [], []
    with mbpe.WordCount(0) as target:
        for _ in range(reps + 1):
            target.reset()
            per_object = []
            for t in tables:
                target.merge(t)
                per_object.append(target.kernel_ms())
            by_object.append(sum(per_object))
            want = target.export()
            target.reset()
            per_blob = []
            t0 = time.perf_counter()
            for b in blobs:
                target.merge(b)
                per_blob.append(target.kernel_ms())
            blob_seconds.append(time.perf_counter() - t0)
            by_blob.append(sum(per_blob))
            assert target.export() == want
        stats, allocations = target.stats(), target.alloc_count()
    return {"kernel_ms_by_object": med(by_object[1:]), "kernel_ms_by_blob": med(by_blob[1:]),
            "kernel_ms_per_table_by_object": per_object, "kernel_ms_per_table_by_blob": per_blob,
            "host_seconds_blob_merges": med(blob_seconds[1:]), "stats": stats, "allocations": allocations}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kinds", default="merge,worst")
    ap.add_argument("--gbytes", type=float, default=1.14)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json")
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "minbpe-cc_amd", "python"))
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import numpy as np
    import torch
    import mbpe
    import oracle as O
    from wordcount_time import _cut
    pattern = O.GPT4_SPLIT_PATTERN
    torch.cuda.set_device(0)
    rows = []

    def emit(row):
        rows.append(row)
        print("#", json.dumps(row), flush=True)

    kinds = args.kinds.split(",")
    if "merge" in kinds:
        with open(os.path.join(DATA, "shakespeare.txt"), "rb") as f:
            small = f.read()
        copies = max(1, int(round(args.gbytes * 1e9 / len(small))))
        data = small * copies
        mbpe.Tokenizer(pattern).train(small, 300, device_split=True)            # code objects loaded, device warm
        pieces = _cut(data, 8)
        tables, add_ms, dedup_ms = [], [], []
        with mbpe.Splitter(pattern) as sp, mbpe.WordCount(0) as one, mbpe.Deduper(0) as dd:
            for rnd in range(args.reps + 1):
                one.reset()
                total_add = total_dd = 0.0
                for k, p in enumerate(pieces):
                    sp.split(np.frombuffer(p, dtype=np.uint8), offsets=False)
                    m_ptr, _, t_ptr = sp.endmask()
                    one.add_endmask(t_ptr, len(p), m_ptr)
                    total_add += one.kernel_ms()
                    dd.chunks_endmask(t_ptr, len(p), m_ptr)
                    total_dd += dd.kernel_ms()
                    if rnd == 0:
                        tables.append(mbpe.WordCount(0))
                        tables[-1].add_endmask(t_ptr, len(p), m_ptr)
                add_ms.append(total_add)
                dedup_ms.append(total_dd)
            want = one.export()
        t0 = time.perf_counter()
        blobs = [t.export() for t in tables]
        export_seconds = time.perf_counter() - t0
        row = merge_rounds(mbpe, tables, blobs, args.reps)
        with mbpe.WordCount(0) as check:
            for b in blobs:
                check.merge(b)
            assert check.export() == want                                       # the merged table is the one object's
        emit({"kind": "merge", "bytes": len(data), "tables": 8, "blob_bytes": [len(b) for b in blobs],
              "export_seconds_8_tables": export_seconds, "add_8_pieces_kernel_ms": med(add_ms[1:]),
              "dedup_alone_8_pieces_kernel_ms": med(dedup_ms[1:]), **row})
        for t in tables:
            t.close()
    if "worst" in kinds:
        n = 256 << 20
        rnd_bytes = np.asarray(O.splitmix64_bytes(42, n), dtype=np.uint8)
        per = n // 4
        off = np.arange(0, per + 1, 8, dtype=np.uint64)
        tables, add_per_piece = [], []
        with mbpe.WordCount(0) as one:
            for k in range(4):
                one.add(rnd_bytes[k * per:(k + 1) * per], off)
                add_per_piece.append(one.kernel_ms())
                tables.append(mbpe.WordCount(0))
                tables[-1].add(rnd_bytes[k * per:(k + 1) * per], off)
            want_stats = one.stats()
        blobs = [t.export() for t in tables]
        row = merge_rounds(mbpe, tables, blobs, args.reps)
        assert row["stats"] == want_stats
        emit({"kind": "worst", "bytes": n, "tables": 4, "blob_bytes": [len(b) for b in blobs],
              "add_kernel_ms_per_piece": add_per_piece, **row})
        for t in tables:
            t.close()
    result = {"gbytes": args.gbytes, "reps": args.reps, "rows": rows}
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
