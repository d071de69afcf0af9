"""The best-fit planners timed (mbpe.pack_fit_plan: the host planner against device=<id>, csrc/pack_fit_dev.hip) on the two
workloads of profiles/r27_pack_fit.md.  Wall time of the whole call, offsets in host memory: the device figure includes
the upload of the offsets and the read-back of len, doc_row and doc_col.  Prints one JSON line per workload.

    python tools/pack_fit_plan_time.py [--device 0] [--repeats 7]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "minbpe-cc_amd", "python"))
import mbpe  # noqa: E402

WORKLOADS = {
    "1M docs of 1..1024 tokens, rows of 2048": lambda rng: (rng.integers(1, 1025, 1_000_000), 2048),
    "1000 docs of 600000 tokens, rows of 512": lambda rng: (np.full(1000, 600_000), 512),
}


def timed(fn, repeats):
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return out, sorted(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    for name, make in WORKLOADS.items():
        lens, S = make(np.random.default_rng(27))
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        mbpe.pack_fit_plan(off[:1001], S, eos_id=2, device=a.device)          # the device is open, the kernels loaded
        host, host_ms = timed(lambda: mbpe.pack_fit_plan(off, S, eos_id=2), a.repeats)
        dev, dev_ms = timed(lambda: mbpe.pack_fit_plan(off, S, eos_id=2, device=a.device), a.repeats)
        same = host["n_rows"] == dev["n_rows"] and all(np.array_equal(host[k], dev[k]) for k in ("lengths", "doc_row", "doc_col"))
        print(json.dumps({"workload": name, "n_rows": int(host["n_rows"]), "same": bool(same),
                          "host_ms": {"min": host_ms[0], "median": host_ms[len(host_ms) // 2], "max": host_ms[-1]},
                          "device_ms": {"min": dev_ms[0], "median": dev_ms[len(dev_ms) // 2], "max": dev_ms[-1]}}))


if __name__ == "__main__":
    main()
