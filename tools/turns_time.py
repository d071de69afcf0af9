"""Multi-turn conversations on the device (csrc/turns.hip) timed.  Every step below runs in a child process of its own
under its own time limit; when one fails, nothing after it is started.

  chat      mbpe_turns_tokens (drop_oldest, a turn-end id, an end id, targets written) over 32-bit tokens in device
            memory into device memory (mbpe_turns_kernel_ms: all eight launches): conversations of 1 .. 16 turns of
            1 .. 256 tokens, about the token count of textpair_time.py's million pairs, every other turn trained,
            max_tokens 2,048 and head_turns 1.
  long      the same call on 1,000 conversations of four turns of 300,000 tokens, no truncation.
  pairs     textpair_time.py's "short" input -- 1,000,000 pairs of documents of 1 .. 1,024 tokens, cut to 1,024 -- as
            two-turn conversations through mbpe_turns_tokens (right, the second turn trained) in turn with
            mbpe_textpair_tokens (longest_first, as in textpair_time.py; the two rules keep different ids of a pair that
            does not fit, so the times compare, not the streams).
The cost of the batch calls with the stage off is tools/fim_time.py's "encoder" step with --parent-root.

    python tools/turns_time.py --json profiles/r38_turns.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TURN_END, END = 60001, 60003

sys.path[:0] = [os.path.join(ROOT, "minbpe-cc_amd", "python")]


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "all": xs}


def step_stage(args):
    import numpy as np
    import torch
    import mbpe
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(7)
    if args.workload == "chat":
        turns = rng.integers(1, 17, size=940000)
        lens = rng.integers(1, 257, size=int(turns.sum()))
        spec = mbpe.turns_spec(2048, "drop_oldest", head_turns=1, turn_end_id=TURN_END, end_id=END)
    elif args.workload == "long":
        turns, lens = np.full(1000, 4), np.full(4000, 300000)
        spec = mbpe.turns_spec(0, "right", turn_end_id=TURN_END, end_id=END)
    else:
        turns, lens = np.full(1000000, 2), rng.integers(1, 1025, size=2000000)
        spec = mbpe.turns_spec(1024, "right", turn_end_id=TURN_END, end_id=END)
    turn_off = np.concatenate([[0], np.cumsum(turns)]).astype(np.uint64)
    flags = (np.arange(len(lens)) - np.repeat(turn_off[:-1].astype(np.int64), turns)) % 2    # every other turn trained
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    n = int(off[-1])
    tokens = (torch.arange(n, dtype=torch.int64, device=dev) % 50000).to(torch.int32)
    new_off, info = mbpe.turns_plan(off, turn_off, flags, spec)
    n_new = int(new_off[-1])
    pair = mbpe.textpair_spec(1024, "longest_first", sep_ids=(TURN_END,), end_id=END, labels="second")
    n_pair = int(mbpe.textpair_plan(off, pair)[0][-1]) if args.workload == "pairs" else 0
    out = torch.empty(max(n_new, n_pair), dtype=torch.int32, device=dev)
    tgt = torch.empty(max(n_new, n_pair), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    src = dict(tokens_ptr=tokens.data_ptr(), n_tokens=n, token_bits=32)
    dst = dict(out_ptr=out.data_ptr(), targets_ptr=tgt.data_ptr())
    tn_ms, tp_ms = [], []
    for i in range(1 + args.reps):
        if n_pair:
            assert mbpe.textpair_tokens(None, off, pair, **src, **dst, cap=n_pair)[0] == n_pair
            if i:
                tp_ms.append(mbpe.textpair_kernel_ms())
        assert mbpe.turns_tokens(None, off, turn_off, flags, spec, **src, **dst, cap=n_new)[0] == n_new
        if i:
            tn_ms.append(mbpe.turns_kernel_ms())
    # a spot check of the last conversation where nothing of it was dropped or cut: its first turn, then the turn-end id
    if not info[-1].any():
        first = int(turn_off[-2])
        o, s, ln = int(new_off[-2]), int(off[first]), int(lens[first])
        assert torch.equal(out[o:o + ln], tokens[s:s + ln]) and int(out[o + ln]) == TURN_END and int(out[n_new - 1]) == END
    t = statistics.median(tn_ms)
    n_bytes = 4 * n_new * 3 + len(lens) * (17 + 8 + 8 + 41 + 16 + 16) + len(turns) * (32 + 56 + 8 + 16)
    res = {"step": "stage", "workload": args.workload, "device": torch.cuda.get_device_name(0),
           "lib": mbpe.lib().mbpe_version().decode(), "conversations": len(turns), "turns": len(lens), "tokens": n,
           "tokens_joined": n_new, "turns_dropped": int(info[:, 0].sum()), "turns_kernel_ms": spread(tn_ms),
           "turns_bytes": n_bytes, "turns_GBps": n_bytes / t / 1e6}
    if n_pair:
        res.update(textpair_kernel_ms=spread(tp_ms), tokens_joined_textpair=n_pair,
                   ratio_turns_to_textpair=t / statistics.median(tp_ms))
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--step", choices=["stage"])
    ap.add_argument("--workload", choices=["chat", "long", "pairs"], default="chat")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json")
    ap.add_argument("--timeout", type=int, default=240)
    args = ap.parse_args()
    if args.step:
        step_stage(args)
        return 0
    results = []
    for workload in ("chat", "long", "pairs"):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", "stage", "--workload", workload, "--reps", str(args.reps)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
        except subprocess.TimeoutExpired:
            print("workload %s ran into its time limit" % workload, file=sys.stderr)
            break
        if r.returncode != 0:
            print("workload %s failed (%d):\n%s" % (workload, r.returncode, r.stderr[-3000:]), file=sys.stderr)
            break
        results.append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(json.dumps(results[-1]))
        sys.stdout.flush()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)
    return 0 if len(results) == 3 else 1


if __name__ == "__main__":
    sys.exit(main())
