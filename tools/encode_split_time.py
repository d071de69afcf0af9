"""Encode with the split on the device (mbpe_splitter_split_docs + mbpe_encoder_encode_endmask) timed against encode with
the split on the host, which stays the default.  Every step below runs in a child process of its own under its own time
limit; when one fails, nothing after it is started.

  split     per text: device time of k_split_find (mbpe_splitter_find_ms) and of the whole split_docs call
            (mbpe_splitter_kernel_ms), wall clock of the call, warm, --reps calls; ranges, chunks, host spans.
  encode    per text, a process each: wall clock of Tokenizer.encode(text, device=0) with device_split False and True,
            alternately, --reps each after one warm call of either; the tokens of the two must be equal.

Texts: shakespeare x --shakespeare-rep, taylorswift x --taylor-rep, and the first with <|endoftext|> after every 4 KiB.
The tokenizer is the gpt4 golden model of taylorswift with the special tokens of special1.txt.

    python tools/encode_split_time.py --md profiles/r12_encode_split.md
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
GOLDEN = os.path.join(ROOT, "tests", "golden")
DATA = os.path.join(GOLDEN, "data")
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "minbpe-cc_amd", "python")]

EOT = b"<|endoftext|>"
TEXTS = ("shakespeare", "taylorswift", "shakespeare+eot")


def text_of(which, args):
    import numpy as np
    name, rep = ("taylorswift.txt", args.taylor_rep) if which == "taylorswift" else ("shakespeare.txt", args.shakespeare_rep)
    one = np.frombuffer(open(os.path.join(DATA, name), "rb").read(), dtype=np.uint8)
    text = np.tile(one, rep)
    label = "%s x %d" % (name, rep)
    if which == "shakespeare+eot":
        n_rows = len(text) // 4096
        body = text[:n_rows * 4096].reshape(n_rows, 4096)
        tail = np.broadcast_to(np.frombuffer(EOT, dtype=np.uint8), (n_rows, len(EOT)))
        text = np.concatenate([np.concatenate([body, tail], axis=1).reshape(-1), text[n_rows * 4096:]])
        label += ", the endoftext token after every 4 KiB"
    return label, text


def tokenizer():
    import mbpe
    import oracle as O
    tok = mbpe.Tokenizer(O.GPT4_SPLIT_PATTERN)
    tok.set_special_tokens_from_file(open(os.path.join(DATA, "special1.txt"), "rb").read())
    tok.set_merges(O.parse_model(open(os.path.join(GOLDEN, "taylorswift_gpt4_lexical_512.model"), "rb").read())[2])
    return tok


def step_split(args):
    import mbpe
    rows = []
    names = [line.split()[0] for line in open(os.path.join(DATA, "special1.txt"), "rb").read().splitlines() if line.strip()]
    for which in TEXTS:
        label, text = text_of(which, args)
        row = {"text": label, "bytes": len(text), "find_ms": [], "kernel_ms": [], "wall_s": []}
        with mbpe.Splitter(mbpe.split_pattern("gpt4")) as sp:
            for i in range(1 + args.reps):
                t = time.perf_counter()
                n_chunks, ranges = sp.split_docs(text, [0, len(text)], names)
                wall = time.perf_counter() - t
                if i:
                    row["find_ms"].append(sp.find_ms())
                    row["kernel_ms"].append(sp.kernel_ms())
                    row["wall_s"].append(wall)
            row["chunks"], row["ranges"] = n_chunks, len(ranges)
            row["host_spans"], row["host_bytes"] = sp.host_spans()
        rows.append(row)
    print(json.dumps({"lib": mbpe.lib().mbpe_version().decode(), "rows": rows}))


def step_encode(args):
    import mbpe
    label, text = text_of(args.text, args)
    tok = tokenizer()
    row = {"text": label, "bytes": len(text), "host_split_s": [], "device_split_s": []}
    want = None
    for i in range(1 + args.reps):
        for key, dev_split in (("host_split_s", False), ("device_split_s", True)):
            t = time.perf_counter()
            got = tok.encode(text, device=0, device_split=dev_split)
            wall = time.perf_counter() - t
            if i:
                row[key].append(wall)
            if want is None:
                want = got
            assert len(got) == len(want) and (got == want).all(), "the two encodes disagree"
    row["tokens"] = len(want)
    print(json.dumps({"lib": mbpe.lib().mbpe_version().decode(), "row": row}))


STEPS = {"split": step_split, "encode": step_encode}


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
    out = ["# Encode with the split on the device, timed (tools/encode_split_time.py)", "",
           "`%s`; %d timed repeats after one warm call; median (min .. max)." % (res["split"]["lib"], args.reps), "",
           "## mbpe_splitter_split_docs alone (one document, the five names of special1.txt)", "",
           "| text | bytes | chunks | ranges | host spans | bytes in host spans | k_split_find, ms | all kernels, ms | "
           "whole call, s |", "|---|---|---|---|---|---|---|---|---|"]
    for r in res["split"]["rows"]:
        out.append("| %s | %d | %d | %d | %d | %d | %s | %s | %s |" % (
            r["text"], r["bytes"], r["chunks"], r["ranges"], r["host_spans"], r["host_bytes"], spread(r["find_ms"]),
            spread(r["kernel_ms"]), spread(r["wall_s"])))
    out += ["", "## Tokenizer.encode(text, device=0) end to end, the two variants alternating", "",
            "| text | tokens | host split, s | device split, s | factor (medians) | faster by more than the spread |",
            "|---|---|---|---|---|---|"]
    for r in res["encode"]:
        h, d = r["host_split_s"], r["device_split_s"]
        out.append("| %s | %d | %s | %s | %.2f | %s |" % (r["text"], r["tokens"], spread(h), spread(d),
                                                            statistics.median(h) / statistics.median(d),
                                                            "yes" if max(d) < min(h) else "NO"))
    out += ["", "\"Faster by more than the spread\": the slowest device-split run is faster than the fastest host-split run "
            "of the same process.", ""]
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEPS))
    ap.add_argument("--text", choices=TEXTS)
    ap.add_argument("--shakespeare-rep", type=int, default=1024)
    ap.add_argument("--taylor-rep", type=int, default=6000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=400, help="seconds per step")
    ap.add_argument("--json")
    ap.add_argument("--md")
    args = ap.parse_args()
    if args.step:
        STEPS[args.step](args)
        return 0
    size = ["--shakespeare-rep", str(args.shakespeare_rep), "--taylor-rep", str(args.taylor_rep), "--reps", str(args.reps)]
    res = {"split": child("split", args.limit, size), "encode": []}
    if res["split"] is None:
        return 1
    print(json.dumps(res["split"]), flush=True)
    for which in TEXTS:
        r = child("encode", args.limit, size + ["--text", which])
        if r is None:
            return 1
        print(json.dumps(r), flush=True)
        res["encode"].append(r["row"])
        if args.json:
            with open(args.json, "w") as f:
                json.dump(res, f, indent=1)
    if args.md:
        with open(args.md, "w") as f:
            f.write(markdown(res, args))
    return 0


if __name__ == "__main__":
    sys.exit(main())
