"""The 32-bit loop (csrc/wide.hip) with the `first` tie-break against the lexical one, on the same corpus: ms per merge
of the 32-bit loop in each mode (mbpe_stats.ms_steps, HIP events around every group of merges; the conversion and
table growth are outside them), and for `first` how many merges needed the position scan (several pairs at the
maximal count) and how far into the stream their earliest tied pair lay (a replay on a second run, one merge per call:
the scan reads at least the stream up to that pair's span and at most that plus one span per wave of its grid).

    python tools/wide_first_time.py [--json out.json]          (from the repository root, on a GPU)
"""
import argparse
import json
import sys
import time

sys.path[:0] = ["tests", "oracle", "minbpe-cc_amd/python"]
import numpy as np  # noqa: E402

import mbpe  # noqa: E402
import oracle as O  # noqa: E402
from test_gpu_wide import _word_corpus  # noqa: E402

SPAN = 1024                 # kSpan (csrc/span.h)
POS_WAVES = 1024 * 4        # k_wide_first_pos: at most 1,024 workgroups of 4 waves


def corpora():
    words, _ = _word_corpus(78, 4200, 24, (6, 14))
    yield "words_78_4200x24", words, 68000, -1                     # hand-over where the slot format ends
    yield "splitmix64_16MiB", O.splitmix64_bytes(7, 16 << 20), 256 + 3000 + 1000, 3000


def timed(tr, data, vocab, wide_from, first):
    tr.set_option("conflict_resolution", 0 if first else 1)
    tr.set_option("first_wide", 1)
    tr.set_option("wide_from", wide_from)
    tr.load_corpus(data)
    tr.train_begin(vocab)
    n16 = (min(256 + wide_from, 65534) if wide_from >= 0 else 65534) - 256
    assert tr.train_steps(n16) == n16
    ms0 = tr.stats()["ms_steps"]
    t = time.time()
    done = tr.train_steps(vocab - 256 - n16)
    wall = time.time() - t
    st = tr.stats()
    m, c = tr.train_result()
    return {"merges_32bit": done, "ms_32bit": st["ms_steps"] - ms0, "wall_s_32bit": wall,
            "ms_per_merge": (st["ms_steps"] - ms0) / max(done, 1), "n_tokens_after": st["n_live"],
            "last_count": int(c[-1]) if len(c) else 0}, m


def replay(tr, data, vocab, wide_from, n_wide, max_samples=100):
    """`first` again, one merge per call through the 32-bit part: at sampled merges, is the maximum tied, and where
    does the earliest tied pair start?"""
    tr.set_option("conflict_resolution", 0)
    tr.set_option("first_wide", 1)
    tr.set_option("wide_from", wide_from)
    tr.load_corpus(data)
    tr.train_begin(vocab)
    n16 = (min(256 + wide_from, 65534) if wide_from >= 0 else 65534) - 256
    assert tr.train_steps(n16) == n16
    every = max(1, n_wide // max_samples)
    samples = tied = 0
    lo_frac, hi_frac = [], []
    for j in range(n_wide):
        if j % every == 0:
            a, b, c = tr.pairs()
            M = int(c.max())
            keys = (a.astype(np.uint64) << np.uint64(32)) | b.astype(np.uint64)
            tk = keys[c == M]
            samples += 1
            if len(tk) > 1:
                tied += 1
                toks, _ = tr.stream()
                t64 = toks.astype(np.uint64)
                pk = (t64[:-1] << np.uint64(32)) | t64[1:]
                pos = int(np.flatnonzero(np.isin(pk, tk))[0])
                n = len(toks)
                n_spans = (n + SPAN - 1) // SPAN
                s = pos // SPAN
                lo_frac.append(min(n, (s + 1) * SPAN) / n)
                hi_frac.append(min(n_spans, s + 1 + POS_WAVES) / n_spans)
        if tr.train_steps(1) != 1:
            break
    return {"sampled_merges": samples, "every": every, "tied": tied,
            "tied_share": tied / max(samples, 1),
            "scan_read_frac_min_mean": float(np.mean(lo_frac)) if lo_frac else 0.0,
            "scan_read_frac_max_mean": float(np.mean(hi_frac)) if hi_frac else 0.0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--no-replay", action="store_true")
    ap.add_argument("--only", choices=("lexical", "first"), help="time one mode only (for a profiler run)")
    args = ap.parse_args()
    out = {}
    with mbpe.Trainer(0) as tr:
        for name, data, vocab, wf in corpora():
            r = {"bytes": len(data), "vocab": vocab, "wide_from": wf}
            for mode in ("lexical", "first"):
                if args.only in (None, mode):
                    r[mode], _ = timed(tr, data, vocab, wf, mode == "first")
            if args.only:
                out[name] = r
                print(name, json.dumps(r), flush=True)
                continue
            r["first_over_lexical"] = r["first"]["ms_per_merge"] / max(r["lexical"]["ms_per_merge"], 1e-9)
            if not args.no_replay:
                r["first_scan"] = replay(tr, data, vocab, wf, r["first"]["merges_32bit"])
            out[name] = r
            print(name, json.dumps(r), flush=True)
    for name, r in out.items():
        if args.only:
            break
        print("%-18s 32-bit loop ms/merge: lexical %.4f (%d merges)  first %.4f (%d merges)  ratio %.2f" % (
            name, r["lexical"]["ms_per_merge"], r["lexical"]["merges_32bit"], r["first"]["ms_per_merge"],
            r["first"]["merges_32bit"], r["first_over_lexical"]))
        if "first_scan" in r:
            s = r["first_scan"]
            print("%-18s position scan ran at %d of %d sampled merges (%.0f%%); stream read before stopping: "
                  "mean %.3f .. %.3f" % (name, s["tied"], s["sampled_merges"], 100 * s["tied_share"],
                                         s["scan_read_frac_min_mean"], s["scan_read_frac_max_mean"]))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
