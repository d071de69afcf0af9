#!/usr/bin/env python3
"""Timing of the token frequency tables (csrc/hist.hip; profiles/r26_token_counts.md).

The texts of r20 / r21 (tests/golden/data/<name>.txt repeated to about --gbytes GB, gpt4 pattern, split on the device,
the merges of the committed 512-entry model of that text).  Jobs, each a child process of its own:

  raw       mbpe_token_counts over tokens that are on the device, table on the device, kernel ms
            (mbpe_token_counts_kernel_ms), warm, median of --reps with min and max, for three inputs of the same length:
            the tokens of the text (encode_endmask in greedy order, flags and all), a uniform draw over 2^17 ids, and
            all tokens equal (the cliff).  GB/s read, and the fraction of one plain read of the same bytes: half the
            time of a device-to-device copy of them (tools/decode_time.py's probe: a copy reads and writes).
  sweep     the same three inputs through stand-alone builds of hist.hip with kHistLocalIds = 2^13, 2^14 and 2^15
            (--build-sweep DIR compiles them, on any machine with hipcc; --sweep-dir DIR names them for the run)
  encoder   Encoder.count_endmask kernel ms against the query call Encoder.encode_endmask(query=True) on the same
            encoder, both orders, dedup off and on, every text; with --parent-root the parent build's query too,
            alternately (the parent has no count call)
  tokenizer end to end on the host clock: Tokenizer.token_counts(device_split=True, dedup=True) against
            Tokenizer.encode(device=0, device_split=True, dedup=True) + np.bincount, both orders

    python tools/token_counts_time.py --build-sweep build/hist_sweep
    python tools/token_counts_time.py --sweep-dir build/hist_sweep --parent-root <parent checkout, built> --json profiles/r26_token_counts.json
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "data")
GOLDEN = os.path.join(ROOT, "tests", "golden")
MODELS = {"shakespeare": "shakespeare_gpt4_lexical_512", "taylorswift": "taylorswift_gpt4_lexical_512"}
SWEEP_BITS = (13, 14, 15)


def _text(name, gbytes):
    with open(os.path.join(DATA, name + ".txt"), "rb") as f:
        one = f.read()
    return one * max(1, int(round(gbytes * 1e9 / len(one))))


def _med(ms):
    ms = sorted(ms)
    return {"median": ms[len(ms) // 2], "min": ms[0], "max": ms[-1]}


def build_sweep(out_dir):
    os.makedirs(out_dir, exist_ok=True)
    pkg = os.path.join(ROOT, "minbpe-cc_amd")
    for bits in SWEEP_BITS:
        subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17",
                               "-fPIC", "-shared", "-fvisibility=hidden", "-DMBPE_HIST_LOCAL_BITS=%d" % bits,
                               "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(pkg, "csrc"),
                               "-I" + os.path.join(pkg, "host"), os.path.join(pkg, "csrc", "hist.hip"),
                               os.path.join(pkg, "host", "errors.cpp"), "-o", os.path.join(out_dir, "libhist_%d.so" % bits)])


def worker(args):
    pkg = args.pkg_root or ROOT
    sys.path.insert(0, os.path.join(pkg, "minbpe-cc_amd", "python"))
    sys.path.insert(0, os.path.join(pkg, "oracle"))
    import numpy as np
    import torch
    import mbpe
    import oracle as O
    pattern = O.GPT4_SPLIT_PATTERN
    dev = torch.device("cuda", 0)
    has_count = "mbpe_encoder_count_endmask" in mbpe.EXPORTS
    with open(os.path.join(GOLDEN, MODELS[args.text] + ".model"), "rb") as f:
        merges = O.parse_model(f.read())[2]
    out = {"job": args.job, "text": args.text, "rows": []}

    def emit(row):
        out["rows"].append(row)
        print("#", json.dumps(row), flush=True)

    def copy_ms(n_bytes):
        src = torch.empty(n_bytes, dtype=torch.uint8, device=dev)
        dst = torch.empty(n_bytes, dtype=torch.uint8, device=dev)
        src.fill_(7)
        ms = []
        for _ in range(args.reps + 3):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            dst.copy_(src)
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        return _med(ms[3:])["median"]

    if args.job in ("raw", "sweep"):
        data = _text(args.text, args.gbytes)
        with mbpe.Splitter(pattern) as sp, mbpe.Encoder(merges) as enc:
            sp.split(data, offsets=False)
            m_ptr, _, t_ptr = sp.endmask()
            buf = torch.empty(len(data), dtype=torch.int32, device=dev)
            n = enc.encode_endmask(t_ptr, len(data), m_ptr, out_ptr=buf.data_ptr(), cap=len(data))[0]
        inputs = [("text tokens (%s, flagged)" % args.text, buf[:n], 512),
                  ("uniform over 2^17 ids", torch.randint(0, 1 << 17, (n,), dtype=torch.int32, device=dev), 1 << 17),
                  ("all tokens equal (id 5)", torch.full((n,), 5, dtype=torch.int32, device=dev), 512)]
        read_ms = copy_ms(4 * n) / 2
        table = torch.zeros(1 << 17, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        if args.job == "raw":
            libs = [(None, mbpe.lib())]
        else:
            libs = [(bits, ctypes.CDLL(os.path.join(args.sweep_dir, "libhist_%d.so" % bits))) for bits in SWEEP_BITS]
        vp, u64, u32, i32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
        for bits, L in libs:
            L.mbpe_token_counts.argtypes = [i32, vp, u64, u32, i32, vp, u64, i32, vp]
            L.mbpe_token_counts_kernel_ms.argtypes = [vp]
            for label, t, n_ids in inputs:
                ms, other, k = [], u64(), ctypes.c_float()
                for _ in range(args.reps + 1):
                    rc = L.mbpe_token_counts(0, vp(t.data_ptr()), n, 32, 1, vp(table.data_ptr()), n_ids, 1, ctypes.byref(other))
                    if rc != 0:
                        sys.exit("mbpe_token_counts failed: %d" % rc)
                    L.mbpe_token_counts_kernel_ms(ctypes.byref(k))
                    ms.append(k.value)
                m = _med(ms[1:])
                assert int(table[:n_ids].sum().item()) + other.value == n
                emit({"case": label, "local_bits": bits, "tokens": n, "n_ids": n_ids, "kernel_ms": m,
                      "gb_per_s": 4 * n / m["median"] / 1e6, "plain_read_ms": read_ms,
                      "fraction_of_plain_read": read_ms / m["median"], "measured": True})
    elif args.job == "encoder":
        data = _text(args.text, args.gbytes)
        with mbpe.Splitter(pattern) as sp:
            out["chunks"] = sp.split(data, offsets=False)
            m_ptr, _, t_ptr = sp.endmask()
            for order in ("greedy", "rank"):
                for dedup in (False, True):
                    with mbpe.Encoder(merges, rank_order=order == "rank", dedup=dedup) as enc:
                        calls = [("query", lambda: enc.encode_endmask(t_ptr, len(data), m_ptr, query=True)[0])]
                        if has_count:
                            calls.append(("count", lambda: enc.count_endmask(t_ptr, len(data), m_ptr)))
                        for what, call in calls:
                            ms = []
                            for _ in range(args.reps + 1):
                                n = call()
                                ms.append(enc.kernel_ms())
                            emit({"case": args.text, "call": what, "order": order, "dedup": dedup, "bytes": len(data),
                                  "tokens": n, "kernel_ms": _med(ms[1:]), "measured": True})
    elif args.job == "tokenizer":
        data = _text(args.text, args.gbytes)
        tok = mbpe.Tokenizer(pattern)
        tok.set_merges(merges)
        tok.encode(data[:1 << 20], device=0, device_split=True)               # code objects loaded, device warm
        for order in ("greedy", "rank"):
            for what in ("encode + bincount", "token_counts"):
                secs = []
                for _ in range(max(args.reps // 2, 2)):
                    t0 = time.perf_counter()
                    if what == "token_counts":
                        got = tok.token_counts([data], device=0, device_split=True, order=order, dedup=True,
                                               batch_bytes=len(data))
                    else:
                        got = np.bincount(tok.encode(data, device=0, device_split=True, order=order, dedup=True),
                                          minlength=256 + len(merges))
                    secs.append(time.perf_counter() - t0)
                emit({"case": what + " " + args.text, "order": order, "bytes": len(data), "tokens": int(got.sum()),
                      "seconds": _med(secs), "measured": True})
        tok.close()
    print(json.dumps(out), flush=True)


def child(pkg_root, job, text, args):
    env = dict(os.environ)
    env.pop("MBPE_LIB", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--pkg-root", pkg_root, "--job", job, "--text", text,
           "--gbytes", str(args.gbytes), "--reps", str(args.reps), "--sweep-dir", args.sweep_dir or ""]
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
    ap.add_argument("--job", default="raw")
    ap.add_argument("--jobs", default="raw,sweep,encoder,tokenizer")
    ap.add_argument("--text", default="shakespeare")
    ap.add_argument("--texts", default="shakespeare,taylorswift")
    ap.add_argument("--gbytes", type=float, default=1.14)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pkg-root", help="(worker) the checkout whose binding and library are timed")
    ap.add_argument("--parent-root", help="checkout of the parent commit with minbpe-cc_amd/libmbpe.so built")
    ap.add_argument("--build-sweep", help="compile the three stand-alone histogram libraries into this directory and stop")
    ap.add_argument("--sweep-dir", help="where --build-sweep left them")
    ap.add_argument("--json")
    args = ap.parse_args()
    if args.build_sweep:
        return build_sweep(args.build_sweep)
    if args.worker:
        return worker(args)
    jobs = args.jobs.split(",")
    texts = args.texts.split(",")
    if "sweep" in jobs and not (args.sweep_dir and os.path.exists(os.path.join(args.sweep_dir, "libhist_13.so"))):
        sys.exit("--sweep-dir must name the directory --build-sweep wrote")
    parent = os.path.abspath(args.parent_root) if args.parent_root else None
    if parent and not os.path.exists(os.path.join(parent, "minbpe-cc_amd", "libmbpe.so")):
        sys.exit("--parent-root must name a checkout of the parent commit with its libmbpe.so built")
    result = {"gbytes": args.gbytes, "reps": args.reps, "runs": []}

    def run(build, job, text):
        result["runs"].append({"build": build, **child(parent if build == "parent" else ROOT, job, text, args)})
        if args.json:                           # kept as it grows: a run that is cut short leaves what it measured
            with open(args.json, "w") as f:
                json.dump(result, f, indent=1)

    if "raw" in jobs:
        run("this", "raw", texts[0])
    if "sweep" in jobs:
        run("this", "sweep", texts[0])
    for text in texts:
        if "encoder" in jobs:
            for build in ("parent", "this", "parent", "this") if parent else ("this",):
                run(build, "encoder", text)
        if "tokenizer" in jobs:
            run("this", "tokenizer", text)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
