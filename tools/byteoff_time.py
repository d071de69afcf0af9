"""Token byte offsets timed (profiles/r18_byteoff.md): mbpe_encoder_kernel_ms of an Encoder call, text and output on
the device, on shakespeare x 1024 with the gpt4 split and the golden gpt4 model, in both orders -- the plain call on
ANOTHER build of the library (--parent-root: a checkout of the parent commit with its libmbpe.so built) and on this
tree's, alternately, every run a fresh process under its own time limit; and the byte-offset call on this tree's, or,
with --parent-byteoff (a parent that has the call: profiles/r22_encode_host.md), on both builds in every run.
Nothing is started after a run that fails.  Every run: 2 warm-up calls, then 15 timed ones.

    python tools/byteoff_time.py --parent-root <checkout of the parent commit> --json byteoff_time.json
"""
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REPS = 15


def child(root, with_boff):
    sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), os.path.join(root, "minbpe-cc_amd", "python"),
                    HERE]
    import numpy as np
    import torch
    import mbpe
    import oracle as O
    from encode_time import tiled, SHAKESPEARE, MODEL
    dev = torch.device("cuda", 0)
    sh = open(SHAKESPEARE, "rb").read()
    merges = O.parse_model(open(MODEL, "rb").read())[2]
    sh_off = mbpe.presplit(O.GPT4_SPLIT_PATTERN, sh)
    rep = 1024
    text = torch.from_numpy(np.frombuffer(sh, dtype=np.uint8).copy()).to(dev).repeat(rep)
    off = tiled(sh_off, len(sh), rep)
    out = torch.empty(len(sh) * rep + 1, dtype=torch.int32, device=dev)
    res = {"root": root, "cases": []}
    with mbpe.Encoder(merges) as enc:
        for rank in (0, 1):
            enc.set_option("rank_order", rank)
            for boff in ((False, True) if with_boff else (False,)):
                kw = {}
                if boff:
                    d_boff = torch.empty(out.numel() + 1, dtype=torch.int64, device=dev)
                    kw = {"byte_off_ptr": d_boff.data_ptr()}
                ms = []
                for k in range(REPS + 2):
                    n = enc.encode_device(text.data_ptr(), text.numel(), off, out.data_ptr(), out.numel(), 32, **kw)
                    if k >= 2:
                        ms.append(enc.kernel_ms())
                if boff:
                    one = enc.encode(sh, sh_off, byte_off=True)[1]
                    got = d_boff[:n + 1].cpu().numpy()
                    assert got[-1] == text.numel() and (got[:len(one)] == one.astype(np.int64)).all()
                    del d_boff
                res["cases"].append({"rank": rank, "byte_off": boff, "tokens": n, "passes": enc.n_passes,
                                     "text_bytes": text.numel(), "ms": ms, "median": statistics.median(ms),
                                     "min": min(ms), "max": max(ms)})
    print("RESULT " + json.dumps(res))


def main():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", required=True)
    ap.add_argument("--json", default="byteoff_time.json")
    ap.add_argument("--parent-byteoff", action="store_true", help="the parent has the byte-offset call: time it there too")
    args = ap.parse_args()
    runs = []
    parent = os.path.abspath(args.parent_root)
    order = ((parent, 0), (ROOT, 0), (parent, 0), (ROOT, 1), (parent, 0), (ROOT, 0))
    if args.parent_byteoff:
        order = ((parent, 1), (ROOT, 1), (parent, 1), (ROOT, 1))
    for root, boff in order:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "child", root, str(boff)], capture_output=True,
                           text=True, timeout=240)
        if r.returncode != 0:
            print(r.stdout[-3000:], r.stderr[-3000:])
            sys.exit(1)                     # nothing more is started after a failure
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
        runs.append(json.loads(line[7:]))
        for c in runs[-1]["cases"]:
            print("parent" if root == parent else "tree", "rank" if c["rank"] else "greedy", "byteoff" if c["byte_off"] else "plain",
                  "median %.3f min %.3f max %.3f ms" % (c["median"], c["min"], c["max"]), "tokens", c["tokens"], flush=True)
        with open(args.json, "w") as f:
            json.dump(runs, f, indent=1)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "child":
        child(sys.argv[2], int(sys.argv[3]))
    else:
        main()
