"""Text pairs on the device (csrc/textpair.hip) timed.  Every step below runs in a child process of its own under its
own time limit; when one fails, nothing after it is started.

  stage     mbpe_textpair_tokens (longest_first, one separator, an end id, targets written) over 32-bit tokens in
            device memory into device memory (mbpe_textpair_kernel_ms: k_textpair_plan, the scan, k_textpair_offsets
            and k_textpair_gather), in turn with mbpe_fim_tokens at rate 0.5 (mbpe_fim_kernel_ms) and mbpe_pack_tokens
            PACKED (mbpe_pack_kernel_ms: k_pack_stream) over the same tokens: "short", 1,000,000 pairs of documents of
            1 .. 1,024 tokens with max_tokens 1,024, and "long", 1,000 pairs of documents of 600,000 tokens with no
            truncation.  All three read and write every token they keep once; textpair writes 4 B of target more.
  end2end   Tokenizer.encode_batch_aux(pairs, textpair=) on 1,000 pairs of lines of shakespeare against the host
            route: encode_batch, truncate longest-first and build the targets in a Python loop, pack_tokens_aux.
The cost of the batch calls with the stage off is tools/fim_time.py's "encoder" step with --parent-root.

    python tools/textpair_time.py --json profiles/r36_textpair.json
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
SEP, END = 60001, 60003

sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "minbpe-cc_amd", "python")]


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "all": xs}


def step_stage(args):
    import numpy as np
    import torch
    import mbpe
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(7)
    if args.workload == "short":
        lens, seq_len, max_tokens = rng.integers(1, 1025, size=2000000), 2048, 1024
    else:
        lens, seq_len, max_tokens = np.full(2000, 600000), 512, 0
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    n = int(off[-1])
    tokens = (torch.arange(n, dtype=torch.int64, device=dev) % 50000).to(torch.int32)
    spec = mbpe.textpair_spec(max_tokens, "longest_first", sep_ids=(SEP,), end_id=END, labels="second")
    fim = mbpe.fim_spec(0.5, 0.5, 60001, 60002, 60003, seed=1)
    new_off, kept = mbpe.textpair_plan(off, spec)
    n_new, n_fim = int(new_off[-1]), int(mbpe.fim_plan(off, fim)[0][-1])
    out = torch.empty(max(n_new, n_fim), dtype=torch.int32, device=dev)
    tgt = torch.empty(n_new, dtype=torch.int32, device=dev)
    n_rows = -(-n // seq_len)
    ids = torch.empty((n_rows, seq_len), dtype=torch.int32, device=dev)
    ln = torch.empty(n_rows, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    src = dict(tokens_ptr=tokens.data_ptr(), n_tokens=n, token_bits=32)
    tp_ms, fim_ms, pack_ms = [], [], []
    for i in range(1 + args.reps):
        assert mbpe.fim_tokens(None, off, fim, **src, out_ptr=out.data_ptr(), cap=n_fim)[0] == n_fim
        f = mbpe.fim_kernel_ms()
        assert mbpe.pack_tokens(None, off, seq_len, layout="packed", **src, out_ptr=ids.data_ptr(), len_ptr=ln.data_ptr(),
                                cap_rows=n_rows) == n_rows
        got = mbpe.textpair_tokens(None, off, spec, **src, out_ptr=out.data_ptr(), targets_ptr=tgt.data_ptr(), cap=n_new)
        assert got[0] == n_new
        if i:
            tp_ms.append(mbpe.textpair_kernel_ms()); fim_ms.append(f); pack_ms.append(mbpe.pack_kernel_ms())
    # a spot check of the last pair: A' (its first a tokens), the separator, B', the end id
    a, b = int(kept[-1][0]), int(kept[-1][1])
    o, sa, sb = int(new_off[-2]), int(off[-3]), int(off[-2])
    assert torch.equal(out[o:o + a], tokens[sa:sa + a]) and int(out[o + a]) == SEP
    assert torch.equal(out[o + a + 1:o + a + 1 + b], tokens[sb:sb + b]) and int(out[n_new - 1]) == END
    t, f, p = statistics.median(tp_ms), statistics.median(fim_ms), statistics.median(pack_ms)
    tp_bytes = 4 * n_new * 3 + len(lens) // 2 * (24 + 24 + 8 + 48)
    print(json.dumps({
        "step": "stage", "workload": args.workload, "device": torch.cuda.get_device_name(0),
        "lib": mbpe.lib().mbpe_version().decode(), "pairs": len(lens) // 2, "tokens": n, "tokens_joined": n_new,
        "textpair_kernel_ms": spread(tp_ms), "fim_kernel_ms": spread(fim_ms), "pack_stream_kernel_ms": spread(pack_ms),
        "ratio_textpair_to_fim": t / f, "ratio_textpair_to_pack": t / p, "textpair_bytes": tp_bytes,
        "textpair_GBps": tp_bytes / t / 1e6}))


def step_end2end(args):
    import numpy as np
    import torch
    import mbpe
    import oracle as O
    pattern, _, merges = O.parse_model(open(MODEL, "rb").read())
    lines = [x for x in open(SHAKESPEARE, "rb").read().splitlines() if len(x) > 20][:2000]
    pairs = list(zip(lines[::2], lines[1::2]))
    tok = mbpe.Tokenizer(pattern)
    tok.set_merges(merges)
    kw = dict(seq_len=32, labels=True, positions=True, segments=True)
    spec = mbpe.textpair_spec(24, "longest_first", sep_ids=(SEP,), end_id=END, labels="second")

    def host_route():
        toks = tok.encode_batch(lines)
        flat, tgt, off = [], [], [0]
        for A, B in zip(toks[::2], toks[1::2]):
            a, b = len(A), len(B)
            while a + b > 22:
                if a > b:
                    a -= 1
                else:
                    b -= 1
            ids = A[:a].tolist() + [SEP] + B[:b].tolist() + [END]
            flat += ids
            tgt += [ids[k + 1] if a <= k < len(ids) - 1 else mbpe.NO_TOKEN for k in range(len(ids))]
            off.append(len(flat))
        return mbpe.pack_tokens_aux(np.array(flat, dtype=np.uint32), off, **kw, label_tokens=np.array(tgt, dtype=np.uint32))

    dev_s, host_s = [], []
    for i in range(1 + args.reps):
        t = time.perf_counter()
        got = tok.encode_batch_aux(pairs, **kw, textpair=spec)
        d = time.perf_counter() - t
        t = time.perf_counter()
        want = host_route()
        h = time.perf_counter() - t
        assert all(np.array_equal(got[k], want[k]) for k in want)
        if i:
            dev_s.append(d); host_s.append(h)
    tok.close()
    print(json.dumps({"step": "end2end", "device": torch.cuda.get_device_name(0), "pairs": len(pairs),
                      "device_route_s": spread(dev_s), "host_route_s": spread(host_s),
                      "ratio_host_to_device": statistics.median(host_s) / statistics.median(dev_s)}))


STEPS = {"stage": step_stage, "end2end": step_end2end}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--step", choices=sorted(STEPS))
    ap.add_argument("--workload", choices=["short", "long"], default="short")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json")
    ap.add_argument("--timeout", type=int, default=240)
    args = ap.parse_args()
    if args.step:
        STEPS[args.step](args)
        return 0
    plan = [("stage", ["--workload", "short"]), ("stage", ["--workload", "long"]), ("end2end", [])]
    results = []
    for step, extra in plan:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--reps", str(args.reps)]
        try:
            r = subprocess.run(cmd + extra, capture_output=True, text=True, timeout=args.timeout)
        except subprocess.TimeoutExpired:
            print("step %s ran into its time limit" % step, file=sys.stderr)
            break
        if r.returncode != 0:
            print("step %s failed (%d):\n%s" % (step, r.returncode, r.stderr[-3000:]), file=sys.stderr)
            break
        results.append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(json.dumps(results[-1]))
        sys.stdout.flush()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)
    return 0 if len(results) == len(plan) else 1


if __name__ == "__main__":
    sys.exit(main())
