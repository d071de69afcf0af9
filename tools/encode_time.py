"""Encode on the device (csrc/encode.hip) timed.  Every step below runs in a child process of its own under its own
time limit; when one fails, nothing after it is started.

  kernel    kernel time of an Encoder call (mbpe_encoder_kernel_ms: HIP events around widen, the passes and the
            finishing kernels; warm, median of --reps), text and output on the device, for shakespeare x 64 and x 1024
            with the gpt4 split and the golden gpt4 model, and for --train-mib MiB of SplitMix64 bytes as ONE chunk
            with a model of --train-vocab ids trained on it by the library.  Bytes moved as the kernels are written:
            a pass over n tokens that leaves n' reads the token array three times (k_enc_cand, k_enc_match and the
            look-ahead of both count once each: 3 x 4n), writes cand twice and reads it twice (4 x 4n) and writes the
            output once (4n'); widen reads n bytes and writes 4n, the finishing kernel reads 4n and writes 4n.  The
            per-pass token counts are the encoder's own (mbpe_encoder_pass_tokens).  With --rank-order every case
            is timed in both orders by one process (option "rank_order" 0, then 1, on the same encoder and buffers): a
            rank pass adds k_enc_rank_sum (reads tokens and cand: 2 x 4n) and k_enc_rank_filter (reads both, writes
            cand: 3 x 4n) to the bytes above, and the one-chunk case makes one pass per merge that applies -- choose
            --train-vocab accordingly.
  wall      wall clock, host text in, host tokens out, of a repeated Encoder.encode against the one-shot
            mbpe.encode_chunks of ANOTHER build of the library (--parent-root: a checkout of the parent commit with its
            libmbpe.so built), same inputs, shakespeare x 1, x 16, x 256; the two are run alternately, --rounds
            processes each.  Condition: the median of the encoder's calls is not above the median of the parent's by
            more than the parent's own min-max spread.
  batch     Tokenizer.encode_batch of shakespeare cut into its lines against a Python loop of
            Tokenizer.encode(line, device=0) on the same build.

    python tools/encode_time.py --parent-root <checkout of the parent commit> --json profiles/r07_encode.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PEAK_BYTES_PER_S = 8e12
SHAKESPEARE = os.path.join(ROOT, "tests", "golden", "data", "shakespeare.txt")
MODEL = os.path.join(ROOT, "tests", "golden", "shakespeare_gpt4_lexical_512.model")


def use_tree(root):
    sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), os.path.join(root, "minbpe-cc_amd", "python")]


def tiled(sh_off, n_sh, rep):
    """Chunk offsets of shakespeare x rep: the split of one copy, repeated (chunks never interact)."""
    import numpy as np
    off = np.empty(rep * (len(sh_off) - 1) + 1, dtype=np.uint64)
    off[0] = 0
    body = sh_off[1:].astype(np.uint64)
    k = len(body)
    for r in range(rep):
        off[1 + r * k:1 + (r + 1) * k] = body + np.uint64(r * n_sh)
    return off


def bytes_moved(n_bytes, pass_tokens, n_out, out_bytes_per_token, rank_order=False):
    passes = 0
    for k, n in enumerate(pass_tokens):
        nxt = pass_tokens[k + 1] if k + 1 < len(pass_tokens) else n_out
        passes += (48 if rank_order else 28) * n + 4 * nxt
    widen = n_bytes + n_bytes // 8 + 4 * n_bytes
    finish = 4 * n_out + out_bytes_per_token * n_out
    return passes, widen + finish


def kernel_case(name, enc, text_t, off, out_t, reps, torch, rank_order=False):
    n_bytes = text_t.numel()
    enc.set_option("rank_order", int(rank_order))
    name += "_rank" if rank_order else ""

    def run():
        n = enc.encode_device(text_t.data_ptr(), n_bytes, off, out_t.data_ptr(), out_t.numel(), 32)
        return n, enc.kernel_ms()
    for _ in range(2):
        n_out, _ = run()
    ms = [run()[1] for _ in range(reps)]
    k = statistics.median(ms)
    pt = enc.pass_tokens()
    in_passes, around = bytes_moved(n_bytes, pt, n_out, 4, rank_order)
    return {"case": name, "order": "rank" if rank_order else "greedy", "kernel_ms_per_pass": k / max(len(pt), 1), "text_bytes": n_bytes, "chunks": 1 if off is None else len(off) - 1, "tokens": n_out,
            "passes": enc.n_passes, "pass_tokens": pt, "reps": reps, "kernel_ms_median": k, "kernel_ms_min": min(ms),
            "kernel_ms_max": max(ms), "text_GBps": n_bytes / k / 1e6, "bytes_moved_passes": in_passes,
            "bytes_moved_widen_finish": around, "bytes_per_pass_mean": in_passes / max(len(pt), 1),
            "share_of_8TBps": (in_passes + around) / (k * 1e-3) / PEAK_BYTES_PER_S}


def step_kernel(args):
    use_tree(ROOT)
    import numpy as np
    import torch
    import mbpe
    import oracle as O
    dev = torch.device("cuda", 0)
    sh = open(SHAKESPEARE, "rb").read()
    merges = O.parse_model(open(MODEL, "rb").read())[2]
    sh_off = mbpe.presplit(O.GPT4_SPLIT_PATTERN, sh)
    res = {"device": torch.cuda.get_device_name(0), "cases": []}
    with mbpe.Encoder(merges) as enc:
        for rep in (64, 1024):
            text = torch.from_numpy(np.frombuffer(sh, dtype=np.uint8).copy()).to(dev).repeat(rep)
            off = tiled(sh_off, len(sh), rep)
            out = torch.empty(len(sh) * rep + 1, dtype=torch.int32, device=dev)
            for rank_order in ((False, True) if args.rank_order else (False,)):
                enc.set_option("rank_order", int(rank_order))
                one = enc.encode(sh, sh_off)
                case = kernel_case("shakespeare_x%d_gpt4_512" % rep, enc, text, off, out,
                                   args.reps if rep == 64 else max(args.reps // 2, 3), torch, rank_order)
                got = out[:len(one) * rep].view(rep, len(one)) & 0x7FFFFFFF
                assert case["tokens"] == len(one) * rep
                assert bool((got == torch.from_numpy(one.view(np.int32)).to(dev)).all()), "tiles differ from one copy"
                res["cases"].append(case)
                del got
            del text, out
            torch.cuda.empty_cache()
    print(json.dumps(res))


def step_splitmix(args):
    use_tree(ROOT)
    import numpy as np
    import torch
    import mbpe
    import oracle as O
    dev = torch.device("cuda", 0)
    data = O.splitmix64_bytes(42, args.train_mib << 20)
    t = time.perf_counter()
    with mbpe.Trainer(0) as tr:
        m = tr.train_lexical(data, args.train_vocab)[0]
    train_s = time.perf_counter() - t
    text = torch.from_numpy(data).to(dev)
    out = torch.empty(len(data), dtype=torch.int32, device=dev)
    cases = []
    with mbpe.Encoder(m) as enc, mbpe.Decoder(m) as dec:
        back = torch.empty(len(data), dtype=torch.uint8, device=dev)
        for rank_order in ((False, True) if args.rank_order else (False,)):
            case = kernel_case("splitmix64_%dMiB_one_chunk_vocab%d" % (args.train_mib, args.train_vocab), enc, text, None,
                               out, max(args.reps // 2, 3), torch, rank_order)
            back.zero_()
            n_back, bad = dec.decode_slots_device(out.data_ptr(), case["tokens"], 32, 0x80000000, None, back.data_ptr(),
                                                  len(data))
            assert (n_back, bad) == (len(data), 0) and bool(torch.equal(back, text)), "decode(encode(text)) != text"
            case["merges"] = len(m)
            case["train_s"] = train_s
            cases.append(case)
    print(json.dumps({"cases": cases}))


def step_wall(args):
    """One process of one build: --api encoder (repeat calls of one Encoder) or oneshot (mbpe.encode_chunks)."""
    use_tree(args.root)
    import numpy as np
    import mbpe
    import oracle as O
    sh = open(SHAKESPEARE, "rb").read()
    merges = O.parse_model(open(MODEL, "rb").read())[2]
    sh_off = mbpe.presplit(O.GPT4_SPLIT_PATTERN, sh)
    rows = []
    enc = mbpe.Encoder(merges) if args.api == "encoder" else None
    for rep in (1, 16, 256):
        data = np.tile(np.frombuffer(sh, dtype=np.uint8), rep)
        off = tiled(sh_off, len(sh), rep)
        f = (lambda: enc.encode(data, off)) if enc else (lambda: mbpe.encode_chunks(data, off, merges)[0])
        first = f()
        f()
        reps = args.reps if rep < 256 else max(args.reps // 3, 3)
        ts = []
        for _ in range(reps):
            t = time.perf_counter()
            got = f()
            ts.append(time.perf_counter() - t)
        assert np.array_equal(got, first)
        import hashlib
        rows.append({"x": rep, "text_bytes": len(data), "tokens": len(got), "seconds": ts,
                     "sha256": hashlib.sha256(got.astype("<u4").tobytes()).hexdigest()})
    print(json.dumps({"api": args.api, "lib": mbpe.LIB_PATH, "version": mbpe.lib().mbpe_version().decode(), "rows": rows}))


def step_batch(args):
    use_tree(ROOT)
    import numpy as np
    import mbpe
    import oracle as O
    sh = open(SHAKESPEARE, "rb").read()
    lines = sh.splitlines(keepends=True)
    tok = mbpe.Tokenizer(O.GPT4_SPLIT_PATTERN)
    tok.set_merges(O.parse_model(open(MODEL, "rb").read())[2])
    tok.encode_batch(lines[:100], device=0)
    ts = []
    for _ in range(3):
        t = time.perf_counter()
        got = tok.encode_batch(lines, device=0)
        ts.append(time.perf_counter() - t)
    t = time.perf_counter()
    loop = [tok.encode(line, device=0) for line in lines]
    loop_s = time.perf_counter() - t
    assert len(got) == len(loop) and all(np.array_equal(a, b) for a, b in zip(got, loop))
    t = time.perf_counter()
    host = [tok.encode(line) for line in lines]
    host_s = time.perf_counter() - t
    assert all(np.array_equal(a, b) for a, b in zip(got, host))
    print(json.dumps({"documents": len(lines), "text_bytes": len(sh), "tokens": int(sum(len(g) for g in got)),
                      "encode_batch_s": ts, "encode_batch_s_median": statistics.median(ts),
                      "python_loop_device_s": loop_s, "python_loop_host_s": host_s}))


STEPS = {"kernel": step_kernel, "splitmix": step_splitmix, "wall": step_wall, "batch": step_batch}


def child(step, limit, extra, log):
    """One step in a fresh process under its own time limit -> its JSON line, or None (and nothing more is run)."""
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step] + extra
    print("+", " ".join(cmd), flush=True)
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT)
    shown = [os.path.relpath(a, ROOT) if os.path.isabs(a) else a for a in extra]
    log.append({"step": step, "args": shown, "exit": p.returncode, "stderr_tail": p.stderr[-2000:] if p.returncode else ""})
    if p.returncode != 0:
        print(p.stderr[-4000:], file=sys.stderr)
        return None
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEPS))
    ap.add_argument("--json")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--train-mib", type=int, default=1024)
    ap.add_argument("--train-vocab", type=int, default=32000)
    ap.add_argument("--parent-root", help="checkout of the parent commit with minbpe-cc_amd/libmbpe.so built")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--api", choices=("encoder", "oneshot"), default="encoder")
    ap.add_argument("--skip", default="", help="comma-separated steps to leave out")
    ap.add_argument("--rank-order", action="store_true",
                    help="kernel and splitmix steps: time every case in rank order too (option \"rank_order\")")
    args = ap.parse_args()
    if args.step:
        import torch
        if not torch.cuda.is_available():
            sys.exit("encode_time.py needs a GPU: there is nothing to time without one")
        return STEPS[args.step](args)

    skip = set(s for s in args.skip.split(",") if s)
    res, log = {}, []
    common = ["--reps", str(args.reps), "--train-mib", str(args.train_mib), "--train-vocab", str(args.train_vocab)]
    common += ["--rank-order"] if args.rank_order else []

    def done():
        res["log"] = log
        print(json.dumps(res))
        if args.json:
            with open(args.json, "w") as f:
                json.dump(res, f, indent=1)

    if "wall" not in skip:
        if not args.parent_root or not os.path.exists(os.path.join(args.parent_root, "minbpe-cc_amd", "libmbpe.so")):
            sys.exit("--parent-root must name a checkout of the parent commit with its libmbpe.so built")
        runs = {"encoder": [], "oneshot": []}
        for _ in range(args.rounds):                     # alternately: this build's encoder, the parent's one-shot call
            for api, root in (("encoder", ROOT), ("oneshot", args.parent_root)):
                r = child("wall", 420, common + ["--api", api, "--root", root], log)
                if r is None:
                    return done()
                runs[api].append(r)
        rows = []
        for i, x in enumerate((1, 16, 256)):
            new = [s for r in runs["encoder"] for s in r["rows"][i]["seconds"]]
            old = [s for r in runs["oneshot"] for s in r["rows"][i]["seconds"]]
            same = len(set(r["rows"][i]["sha256"] for api in runs for r in runs[api])) == 1
            row = {"x": x, "text_bytes": runs["encoder"][0]["rows"][i]["text_bytes"], "tokens": runs["encoder"][0]["rows"][i]["tokens"],
                   "same_tokens": same,
                   "encoder_repeat_s": {"median": statistics.median(new), "min": min(new), "max": max(new), "n": len(new)},
                   "parent_oneshot_s": {"median": statistics.median(old), "min": min(old), "max": max(old), "n": len(old)}}
            row["ratio_parent_over_encoder"] = row["parent_oneshot_s"]["median"] / row["encoder_repeat_s"]["median"]
            row["not_slower"] = same and row["encoder_repeat_s"]["median"] <= row["parent_oneshot_s"]["median"] + (max(old) - min(old))
            rows.append(row)
        res["wall"] = {"parent_version": runs["oneshot"][0]["version"], "version": runs["encoder"][0]["version"], "rows": rows,
                       "pass_not_slower": all(r["not_slower"] for r in rows)}
    for step, limit in (("kernel", 420), ("batch", 300), ("splitmix", 600)):
        if step in skip:
            continue
        r = child(step, limit, common, log)
        if r is None:
            return done()
        if step == "batch":
            res["batch"] = r
        else:
            res.setdefault("kernel", {"cases": []})["cases"] += r["cases"]
            if "device" in r:
                res["device"] = r["device"]
    done()


if __name__ == "__main__":
    main()
