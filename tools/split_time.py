"""The gpt4 pre-split on the device (csrc/split.hip: mbpe_splitter_split) timed against the host split it replaces.
Every step below runs in a child process of its own under its own time limit; when one fails, nothing after it is
started.

  split     per text: device time of the split (mbpe_splitter_kernel_ms: HIP events around its kernels) and wall clock of
            the whole call (upload, kernels, PCRE2 on the host spans), warm, --reps calls; the host-span share; wall
            clock of mbpe_presplit on the same bytes in the same process (the unchanged host code: the baseline).
  train     per text: wall clock of Tokenizer.train (gpt4, vocab 512, lexical) with and without device_split,
            alternately, --reps each; the merges of the two must be equal.

Texts: shakespeare x --shakespeare-rep (pure ASCII) and taylorswift x --taylor-rep (1.2 % of its bytes in host spans),
built by repetition from the fixtures.

--unicode: every text is split twice, with the splitter's option "unicode" off and on, the training runs with
device_split="unicode", and two more texts of --script-mib MiB each join in: the CJK pseudo-text without a space and
the Cyrillic one (tests/split_unicode_cases.py, one MiB of each repeated).  The time PCRE2 took to fill the class
table, once in the process, is reported too.

    python tools/split_time.py --md profiles/r11_split.md
    python tools/split_time.py --unicode --md profiles/r13_split_unicode.md
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DATA = os.path.join(ROOT, "tests", "golden", "data")
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "minbpe-cc_amd", "python"), os.path.join(ROOT, "tests")]


def texts(args):
    import numpy as np
    out = []
    for name, rep in (("shakespeare.txt", args.shakespeare_rep), ("taylorswift.txt", args.taylor_rep)):
        one = np.frombuffer(open(os.path.join(DATA, name), "rb").read(), dtype=np.uint8)
        if rep:
            out.append(("%s x %d" % (name, rep), np.tile(one, rep)))
    if args.unicode and args.script_mib:
        import split_unicode_cases as U
        for name, make in (("cjk", U.cjk), ("cyrillic", U.cyrillic)):
            one = np.frombuffer(make(1 << 20), dtype=np.uint8)
            out.append(("%s pseudo-text, 1 MiB x %d" % (name, args.script_mib), np.tile(one, args.script_mib)))
    return out


def step_split(args):
    import mbpe
    L = mbpe.lib()
    pat = mbpe.split_pattern("gpt4")
    rows = []
    table_ms = mbpe.split_unicode_table()[2] if args.unicode else None
    for name, text in texts(args):
        for unicode in ((0, 1) if args.unicode else (0,)):
            row = {"text": name, "unicode": unicode, "bytes": len(text), "kernel_ms": [], "split_wall_s": [],
                   "presplit_wall_s": []}
            with mbpe.Splitter(pat) as sp:
                if unicode:
                    sp.set_option("unicode", 1)
                for i in range(1 + args.reps):
                    t = time.perf_counter()
                    n_chunks = sp.split(text, offsets=False)
                    wall = time.perf_counter() - t
                    if i:
                        row["kernel_ms"].append(sp.kernel_ms())
                        row["split_wall_s"].append(wall)
                row["chunks"] = n_chunks
                row["host_spans"], row["host_bytes"] = sp.host_spans()
            for _ in range(0 if unicode else args.host_reps):       # (the host split is timed once per text)
                h = ctypes.c_void_p()
                t = time.perf_counter()
                rc = L.mbpe_presplit(pat.encode(), text.ctypes.data, len(text), ctypes.byref(h))
                row["presplit_wall_s"].append(time.perf_counter() - t)
                assert rc == 0 and L.mbpe_split_count(h) == n_chunks, "the two splits disagree on the number of chunks"
                L.mbpe_split_free(h)
            rows.append(row)
    print(json.dumps({"lib": L.mbpe_version().decode(), "table_ms": table_ms, "rows": rows}))


def step_train(args):
    import mbpe
    pat = mbpe.split_pattern("gpt4")
    rows = []
    for name, text in texts(args):
        row = {"text": name, "bytes": len(text), "host_split_s": [], "device_split_s": []}
        merges = {}
        for i in range(args.reps):
            for key, dev_split in (("host_split_s", False), ("device_split_s", "unicode" if args.unicode else True)):
                tok = mbpe.Tokenizer(pat)
                t = time.perf_counter()
                tok.train(text, 512, device_split=dev_split)
                row[key].append(time.perf_counter() - t)
                merges[key] = tok.merges().tolist()
                tok.close()
            assert merges["host_split_s"] == merges["device_split_s"], "the two trainings disagree"
        rows.append(row)
    print(json.dumps({"lib": mbpe.lib().mbpe_version().decode(), "rows": rows}))


STEPS = {"split": step_split, "train": step_train}


def child(step, limit, extra):
    """One step in a fresh process under its own time limit -> its JSON line, or None (and nothing more is run)."""
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step] + extra
    print("+", " ".join(cmd), flush=True)
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT)
    if p.returncode != 0:
        print("step %s ended with status %d\n%s" % (step, p.returncode, p.stderr[-4000:]), flush=True)
        return None
    return json.loads(p.stdout.strip().splitlines()[-1])


def spread(xs):
    return "%.3f (%.3f .. %.3f)" % (statistics.median(xs), min(xs), max(xs))


def markdown(res, args):
    out = ["# The gpt4 pre-split on the device, timed (tools/split_time.py)", "",
           "`%s`; %d timed repeats after one warm call; median (min .. max)." % (res["split"]["lib"], args.reps), "",
           "## The split alone", "",
           "| text | bytes | chunks | host spans | bytes in host spans | device time, ms | GB/s of text (device time) | "
           "whole call, s | mbpe_presplit, s |", "|---|---|---|---|---|---|---|---|---|"]
    for r in res["split"]["rows"]:
        out.append("| %s | %d | %d | %d | %d (%.2f %%) | %s | %.1f | %s | %s |" % (
            r["text"] + (", unicode on" if r.get("unicode") else ""), r["bytes"], r["chunks"], r["host_spans"],
            r["host_bytes"], 100.0 * r["host_bytes"] / r["bytes"], spread(r["kernel_ms"]),
            r["bytes"] / statistics.median(r["kernel_ms"]) / 1e6, spread(r["split_wall_s"]),
            spread(r["presplit_wall_s"]) if r["presplit_wall_s"] else "(above)"))
    if res["split"].get("table_ms") is not None:
        out += ["", "The class table: PCRE2 filled it in %.1f ms, once in the process." % res["split"]["table_ms"]]
    if "train" not in res:
        return "\n".join(out + [""])
    out += ["", "## Tokenizer.train end to end (gpt4, vocab 512, lexical), the two variants alternating", "",
            "| text | host split, s | device split, s | factor (medians) | faster by more than the spread |",
            "|---|---|---|---|---|"]
    for r in res["train"]["rows"]:
        h, d = r["host_split_s"], r["device_split_s"]
        out.append("| %s | %s | %s | %.2f | %s |" % (r["text"], spread(h), spread(d),
                                                       statistics.median(h) / statistics.median(d),
                                                       "yes" if max(d) < min(h) else "NO"))
    out += ["", "\"Faster by more than the spread\": the slowest device-split run is faster than the fastest host-split run.", ""]
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEPS))
    ap.add_argument("--shakespeare-rep", type=int, default=1024)
    ap.add_argument("--taylor-rep", type=int, default=6000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--unicode", action="store_true", help="the splitter's option \"unicode\": off against on")
    ap.add_argument("--script-mib", type=int, default=1024, help="size of the two pseudo-texts of --unicode (0: none)")
    ap.add_argument("--only", choices=sorted(STEPS), help="run this step alone")
    ap.add_argument("--limit", type=int, default=500, help="seconds per step")
    ap.add_argument("--json")
    ap.add_argument("--md")
    args = ap.parse_args()
    if args.step:
        STEPS[args.step](args)
        return 0
    size = ["--shakespeare-rep", str(args.shakespeare_rep), "--taylor-rep", str(args.taylor_rep), "--reps", str(args.reps),
            "--host-reps", str(args.host_reps), "--script-mib", str(args.script_mib)] + (["--unicode"] if args.unicode else [])
    res = {}
    for step in ([args.only] if args.only else ["split", "train"]):
        res[step] = child(step, args.limit, size)
        if res[step] is None:
            return 1
        print(json.dumps(res[step]), flush=True)
        if args.json:
            with open(args.json, "w") as f:
                json.dump(res, f, indent=1)
    if args.md:
        with open(args.md, "w") as f:
            f.write(markdown(res, args))
    return 0


if __name__ == "__main__":
    sys.exit(main())
