"""Batch decode on the device (csrc/decode.hip: mbpe_decode_batch) timed.  Every step below runs in a child process of
its own under its own time limit; when one fails, nothing after it is started.

  batch     wall clock of Tokenizer.decode_batch of shakespeare cut into its lines (gpt4 split, golden gpt4 model)
            against a Python loop of Tokenizer.decode(tokens, device=0) and against the host loop, same build, same
            process.
  kernel    kernel time (mbpe_decoder_kernel_ms, warm, --reps calls) of mbpe_decode_batch with one document per line
            and of mbpe_decode_tokens on the same flat tokens, alternately, tokens and output on the device, for
            shakespeare x --rep.
  parent    the mbpe_decode_tokens half of `kernel` with ANOTHER build of the library (--parent-root: a checkout of
            the parent commit with its libmbpe.so built).

    python tools/decode_batch_time.py --parent-root <checkout of the parent commit> --json profiles/r08_decode_batch.json
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
SHAKESPEARE = os.path.join(ROOT, "tests", "golden", "data", "shakespeare.txt")
MODEL = os.path.join(ROOT, "tests", "golden", "shakespeare_gpt4_lexical_512.model")


def use_tree(root):
    sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(root or ROOT, "minbpe-cc_amd", "python")]


def tokenizer():
    import mbpe
    import oracle as O
    tok = mbpe.Tokenizer(O.GPT4_SPLIT_PATTERN)
    tok.set_merges(O.parse_model(open(MODEL, "rb").read())[2])
    return tok


def step_batch(args):
    use_tree(args.tree)
    import mbpe
    lines = open(SHAKESPEARE, "rb").read().splitlines(keepends=True)
    tok = tokenizer()
    enc = tok.encode_batch(lines, device=0)
    tok.decode_batch(enc[:100], device=0)
    ts = []
    for _ in range(3):
        t = time.perf_counter()
        got = tok.decode_batch(enc, device=0)
        ts.append(time.perf_counter() - t)
    assert got == lines
    t = time.perf_counter()
    loop = [tok.decode(e, device=0) for e in enc]
    loop_s = time.perf_counter() - t
    t = time.perf_counter()
    host = [tok.decode(e) for e in enc]
    host_s = time.perf_counter() - t
    assert loop == lines and host == lines
    print(json.dumps({"lib": mbpe.lib().mbpe_version().decode(), "documents": len(lines),
                      "tokens": int(sum(len(e) for e in enc)), "text_bytes": sum(len(x) for x in lines),
                      "decode_batch_s": ts, "decode_batch_s_median": statistics.median(ts),
                      "python_loop_device_s": loop_s, "python_loop_host_s": host_s}))


def step_kernel(args):
    use_tree(args.tree)
    import numpy as np
    import torch
    import mbpe
    import oracle as O
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    sh = open(SHAKESPEARE, "rb").read()
    lines = sh.splitlines(keepends=True)
    enc = tokenizer().encode_batch(lines, device=0)
    one = np.concatenate(enc).astype(np.uint32)
    one_off = np.concatenate([[0], np.cumsum([len(e) for e in enc])]).astype(np.uint64)
    rep = args.rep
    tokens = torch.from_numpy(one.view(np.int32)).to(dev).repeat(rep)
    n_tok = tokens.numel()
    off = np.empty(rep * len(lines) + 1, dtype=np.uint64)
    off[0] = 0
    for r in range(rep):
        off[1 + r * len(lines):1 + (r + 1) * len(lines)] = one_off[1:] + np.uint64(r * len(one))
    out = torch.zeros(len(sh) * rep, dtype=torch.uint8, device=dev)
    want_off = np.concatenate([[0], np.cumsum([len(x) for x in lines])]).astype(np.uint64)
    row = {"lib": mbpe.lib().mbpe_version().decode(), "rep": rep, "tokens": n_tok, "documents": len(off) - 1,
           "text_bytes": out.numel(), "tokens_ms": [], "batch_ms": []}
    with mbpe.Decoder(O.parse_model(open(MODEL, "rb").read())[2]) as d:
        def flat():
            assert d.decode_device(tokens.data_ptr(), n_tok, out.data_ptr(), out.numel()) == (out.numel(), 0)
            return d.kernel_ms()

        def batch():
            b, n, bad = d.decode_batch_device(tokens.data_ptr(), n_tok, off, out.data_ptr(), out.numel())
            ms = d.kernel_ms()
            assert (n, bad) == (out.numel(), 0)
            assert np.array_equal(b[:len(want_off)], want_off) and int(b[-1]) == out.numel()
            return ms
        has_batch = hasattr(d, "decode_batch_device") and not args.flat_only
        for i in range(2 + args.reps):
            a = flat()
            b = batch() if has_batch else None
            if i >= 2:
                row["tokens_ms"].append(a)
                if has_batch:
                    row["batch_ms"].append(b)
    first = torch.from_numpy(np.frombuffer(sh, dtype=np.uint8).copy()).to(dev)
    assert bool(torch.equal(out[:len(sh)], first)) and bool(torch.equal(out[-len(sh):], first))
    print(json.dumps(row))


STEPS = {"batch": step_batch, "kernel": step_kernel}


def child(step, limit, extra):
    """One step in a fresh process under its own time limit -> its JSON line, or None (and nothing more is run)."""
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step] + extra
    print("+", " ".join(cmd), flush=True)
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT)
    if p.returncode != 0:
        print("step %s ended with status %d\n%s" % (step, p.returncode, p.stderr[-4000:]), flush=True)
        return None
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEPS))
    ap.add_argument("--rep", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--flat-only", action="store_true")
    ap.add_argument("--tree")
    ap.add_argument("--parent-root")
    ap.add_argument("--json")
    args = ap.parse_args()
    if args.step:
        STEPS[args.step](args)
        return 0
    res = {}
    size = ["--rep", str(args.rep), "--reps", str(args.reps)]
    plan = [("batch", "batch", 300, []), ("kernel", "kernel", 400, size)]
    if args.parent_root:
        plan.append(("parent", "kernel", 400, size + ["--flat-only", "--tree", os.path.abspath(args.parent_root)]))
    for name, step, limit, extra in plan:
        res[name] = child(step, limit, extra)
        if res[name] is None:
            break
        print(json.dumps(res[name]), flush=True)
        if args.json:
            with open(args.json, "w") as f:
                json.dump(res, f, indent=1)
    return 0 if all(res.get(k) is not None for k, *_ in plan) else 1


if __name__ == "__main__":
    sys.exit(main())
