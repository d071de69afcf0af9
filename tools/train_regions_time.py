#!/usr/bin/env python3
"""Timing of the 32-bit training loop with the option "regions" (profiles/r35_train_regions.md).

  r20     the workload of profiles/r20_dedup.md and r32_train_resident.md: tests/golden/data/shakespeare.txt repeated to
          about --gbytes GB, gpt4 pattern, split and deduplicated on the device, the deduper's result loaded with
          Trainer.load_corpus_endmask_weighted, vocab 512 and 10,000, both tie-breaks -- on the parent commit's build
          (--parent-root: a checkout of the parent commit with its libmbpe.so built) and on this one with the option off
          and on at every "region_tokens" of REGION_TOKENS, --rounds times, alternating.  The bar for "off" and for
          "on" is the parent's own spread.
  sweep   the random-chunk corpus of r32 (chunks of at most 12 bytes over 4 letters, deduplicated on the host) at growing
          numbers of unique-chunk tokens, up to a few million, vocab 256 + 2,000, this build off and on (the default
          "region_tokens").

Per configuration: microseconds per merge from mbpe_stats.ms_steps (device events around the groups of merges), the
merges' hash, and with the option on mbpe_train_regions_stats.  Every (build, round) is one child process under its
own timeout.  A run needs a GPU:

    python tools/train_regions_time.py --parent-root <checkout of the parent commit> --json profiles/r35_train_regions.json
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "data")
SWEEP = [2000, 8000, 30000, 60000, 120000, 600000]      # chunks drawn; the unique ones' tokens are what is reported
REGION_TOKENS = [128, 256, 512, 1024, 2048]


def timed(tr, vocab, cr, region_tokens):
    """region_tokens: None = a build without the option, 0 = the option off, else "regions" 1 at that size"""
    tr.set_option("conflict_resolution", cr)
    if region_tokens is not None:
        tr.set_option("regions", 1 if region_tokens else 0)
        if region_tokens:
            tr.set_option("region_tokens", region_tokens)
    tr.train_begin(vocab)
    n0 = len(tr.stream()[0])
    tr.train_steps(vocab - 256)
    m, _ = tr.train_result()
    st = tr.stats()
    row = {"conflict_resolution": "lexical" if cr else "first", "vocab": vocab, "region_tokens": region_tokens,
           "tokens": n0, "merges": len(m), "ms_steps": st["ms_steps"],
           "us_per_merge": 1e3 * st["ms_steps"] / max(len(m), 1), "merges_sha": hashlib.sha256(m.tobytes()).hexdigest()[:16]}
    if region_tokens:
        n_reg, groups, regions_last = tr.regions_stats()
        row.update(regions_merges=n_reg, groups=groups, regions_last=regions_last)
    print("#", json.dumps(row), flush=True)
    return row


def worker(args):
    pkg = args.pkg_root or ROOT                 # the binding and the library of that checkout go together
    sys.path.insert(0, os.path.join(pkg, "minbpe-cc_amd", "python"))
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import mbpe
    import oracle as O
    out = {"rows": [], "sweep": []}
    with open(os.path.join(DATA, "shakespeare.txt"), "rb") as f:
        one = f.read()
    mbpe.Tokenizer(O.GPT4_SPLIT_PATTERN).train(one, 300, device_split=True)      # code objects loaded, device warm
    if args.what == "r20":
        data = one * max(1, int(round(args.gbytes * 1e9 / len(one))))
        with mbpe.Splitter(O.GPT4_SPLIT_PATTERN) as sp, mbpe.Deduper(0) as dd:
            sp.split(data, offsets=False)
            m_ptr, _, t_ptr = sp.endmask()
            nu, nb = dd.chunks_endmask(t_ptr, len(data), m_ptr)
            t_u, m_u, w_u, _ = dd.result()
            out.update(bytes=len(data), n_unique=nu, n_unique_bytes=nb)
            for vocab in (512, 10000):
                for cr in (1, 0):
                    for rt in [None] if args.parent else [0] + REGION_TOKENS:
                        with mbpe.Trainer(0) as tr:
                            tr.load_corpus_endmask_weighted(m_u, text_ptr=t_u, n_bytes=nb, weights_ptr=w_u, n_weights=nu)
                            out["rows"].append(timed(tr, vocab, cr, rt))
    else:
        import dedup_cases as C
        for n_chunks in SWEEP:
            uniq, weights, _ = C.dedup(C.random_chunks(1, n_chunks, 12, 4))
            u_data, u_off = C.join(uniq)
            for cr in (1, 0):
                for rt in [None] if args.parent else [0, args.region_tokens]:
                    with mbpe.Trainer(0) as tr:
                        tr.load_corpus_weighted(u_data, u_off, weights)
                        out["sweep"].append(timed(tr, 256 + 2000, cr, rt))
    print(json.dumps(out), flush=True)


def child(pkg_root, what, parent, args):
    env = dict(os.environ)
    env.pop("MBPE_LIB", None)
    cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--worker",
           "--pkg-root", pkg_root, "--what", what, "--gbytes", str(args.gbytes),
           "--region-tokens", str(args.region_tokens)] + (["--parent"] if parent else [])
    proc = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, text=True)
    last = ""
    for line in proc.stdout:                    # rows are shown as they come
        if line.startswith("#"):
            print(line.rstrip(), flush=True)
        elif line.strip():
            last = line
    if proc.wait() != 0:                        # (a fault, an abort or a time limit: nothing more runs on the device)
        sys.exit("worker failed (%d): %s" % (proc.returncode, last[-2000:]))
    return json.loads(last)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--parent", action="store_true", help="(worker) the parent's build: no regions options")
    ap.add_argument("--what", default="r20", choices=["r20", "sweep"])
    ap.add_argument("--only", choices=["r20", "sweep"], help="one of the two workloads only")
    ap.add_argument("--gbytes", type=float, default=1.14)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--region-tokens", type=int, default=256, help="\"region_tokens\" of the sweep's runs")
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds one child process may take")
    ap.add_argument("--pkg-root", help="(worker) the checkout whose binding and library are timed")
    ap.add_argument("--parent-root", help="checkout of the parent commit with minbpe-cc_amd/libmbpe.so built")
    ap.add_argument("--json")
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    parent_lib = os.path.join(args.parent_root or "", "minbpe-cc_amd", "libmbpe.so")
    if not args.parent_root or not os.path.exists(parent_lib):
        sys.exit("--parent-root must name a checkout of the parent commit with its libmbpe.so built")
    result = {"gbytes": args.gbytes, "runs": []}
    for what in [args.only] if args.only else ["r20", "sweep"]:
        for r in range(args.rounds):
            result["runs"].append({"build": "parent", "what": what, "round": r,
                                   **child(os.path.abspath(args.parent_root), what, True, args)})
            result["runs"].append({"build": "this", "what": what, "round": r, **child(ROOT, what, False, args)})
            if args.json:                       # (kept after every pair of runs: a later failure loses nothing)
                with open(args.json, "w") as f:
                    json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
