"""Span corruption on the device (csrc/denoise.hip) timed.  Every step below runs in a child process of its own under
its own time limit; when one fails, nothing after it is started.

  stage      mbpe_denoise_tokens at T5's defaults (density 0.15, mean 3, 100 sentinels) over 32-bit tokens in device
             memory into device memory (mbpe_denoise_kernel_ms: all kernels of the stage), alternating with
             mbpe_pack_tokens PACKED (mbpe_pack_kernel_ms: k_pack_stream) and mbpe_fim_tokens at rate 0.5
             (mbpe_fim_kernel_ms) over the same tokens, on the two workloads of profiles/r28_fim.md: "short", 1,000,000
             documents of 1 .. 1,024 tokens, one unit each, and "long", 1,000 documents of 600,000 tokens in units of 568.
             Run the step under `rocprofv3 --kernel-trace --stats` for the time kernel by kernel (--reps 3 is enough).
  tokenizer  Tokenizer.encode_batch_denoise end to end (matrices in host memory) against the host route it replaces:
             Tokenizer.encode_batch, the rule in NumPy-free Python (tests/denoise_cases.ref_apply), two pack_tokens.
  aux        Encoder.encode_batch_aux PACKED over shakespeare x --rep with every line a document, without and with
             set_fim, matrices in device memory: what the existing batch calls cost.  Under `rocprofv3 --kernel-trace
             --stats`, once with this library and once with the parent commit's (MBPE_LIB and MBPE_DENOISE_TIME_PKG name
             its library and its Python package), the kernel times of the two are compared.

    python tools/denoise_time.py --json profiles/r30_denoise.json
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
SENT = 60099

sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"),
                os.environ.get("MBPE_DENOISE_TIME_PKG") or os.path.join(ROOT, "minbpe-cc_amd", "python")]


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "all": xs}


def step_stage(args):
    import numpy as np
    import torch
    import mbpe
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(7)
    if args.workload == "short":
        lens, seq_len, seg = rng.integers(1, 1025, size=1000000), 2048, 0
    else:
        lens, seq_len, seg = np.full(1000, 600000), 512, 568
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    n, n_docs = int(off[-1]), len(lens)
    tokens = (torch.arange(n, dtype=torch.int64, device=dev) % 50000).to(torch.int32)
    spec = mbpe.denoise_spec(0.15, 3.0, sentinel_id=SENT, segment_tokens=seg, seed=1)
    in_off, tg_off, unit_doc = mbpe.denoise_plan(off, spec)
    n_in, n_tg, n_units = int(in_off[-1]), int(tg_off[-1]), len(unit_doc)
    d_in = torch.empty(n_in, dtype=torch.int32, device=dev)
    d_tg = torch.empty(n_tg, dtype=torch.int32, device=dev)
    fspec = mbpe.fim_spec(0.5, 0.5, 60001, 60002, 60003, seed=1)
    n_fim = int(mbpe.fim_plan(off, fspec)[0][-1])
    d_fim = torch.empty(n_fim, dtype=torch.int32, device=dev)
    n_rows = -(-n // seq_len)
    ids = torch.empty((n_rows, seq_len), dtype=torch.int32, device=dev)
    ln = torch.empty(n_rows, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    dn_ms, pack_ms, fim_ms, dn_wall = [], [], [], []
    for i in range(1 + args.reps):
        t = time.perf_counter()
        got = mbpe.denoise_tokens(None, off, spec, tokens_ptr=tokens.data_ptr(), n_tokens=n, token_bits=32,
                                  in_ptr=d_in.data_ptr(), cap_in=n_in, tg_ptr=d_tg.data_ptr(), cap_tg=n_tg)
        w = time.perf_counter() - t
        assert got[:2] == (n_in, n_tg)
        rows = mbpe.pack_tokens(None, off, seq_len, layout="packed", tokens_ptr=tokens.data_ptr(), n_tokens=n, token_bits=32,
                                out_ptr=ids.data_ptr(), len_ptr=ln.data_ptr(), cap_rows=n_rows)
        assert rows == n_rows
        got_fim, _ = mbpe.fim_tokens(None, off, fspec, tokens_ptr=tokens.data_ptr(), n_tokens=n, token_bits=32,
                                     out_ptr=d_fim.data_ptr(), cap=n_fim)
        assert got_fim == n_fim
        if i:
            dn_ms.append(mbpe.denoise_kernel_ms()); pack_ms.append(mbpe.pack_kernel_ms())
            fim_ms.append(mbpe.fim_kernel_ms()); dn_wall.append(w)
    # a spot check against the rule in Python: the first unit with noise
    import denoise_cases as D
    s = D.spec(spec.density, spec.mean_span_q8, seed=1, seg=seg, sent=SENT)
    k = int(np.flatnonzero(np.diff(tg_off.astype(np.int64)) > 0)[0])
    d = int(unit_doc[k])
    u = k - int(np.searchsorted(unit_doc, d))
    a = int(off[d]) + u * seg
    L = min(seg, int(off[d + 1]) - a) if seg else int(off[d + 1]) - a
    want_in, want_tg = D.ref_unit(s, d, u, tokens[a:a + L].cpu().tolist())
    assert d_in[int(in_off[k]):int(in_off[k + 1])].cpu().tolist() == want_in
    assert d_tg[int(tg_off[k]):int(tg_off[k + 1])].cpu().tolist() == want_tg
    f, p, m = statistics.median(dn_ms), statistics.median(pack_ms), statistics.median(fim_ms)
    dn_bytes = 4 * n + 4 * (n_in + n_tg) + n_docs * 40 + n_units * 56
    print(json.dumps({
        "step": "stage", "workload": args.workload, "device": torch.cuda.get_device_name(0),
        "lib": mbpe.lib().mbpe_version().decode(), "documents": n_docs, "units": n_units, "tokens": n, "inputs": n_in,
        "targets": n_tg, "segment_tokens": seg, "denoise_kernel_ms": spread(dn_ms), "pack_stream_kernel_ms": spread(pack_ms),
        "fim_kernel_ms": spread(fim_ms), "denoise_wall_s": spread(dn_wall), "ratio_denoise_to_pack": f / p,
        "ratio_denoise_to_fim": f / m, "denoise_bytes": dn_bytes, "denoise_GBps": dn_bytes / f / 1e6}))


def step_tokenizer(args):
    import numpy as np
    import mbpe
    import oracle as O
    import denoise_cases as D
    sh = open(SHAKESPEARE, "rb").read()
    pattern, _, merges = O.parse_model(open(MODEL, "rb").read())
    tok = mbpe.Tokenizer(pattern)
    tok.set_merges(merges)
    lines = sh.splitlines(keepends=True)
    docs = [b"".join(lines[i:i + 40]) for i in range(0, len(lines), 40)] * args.rep    # paragraphs of 40 lines
    spec = mbpe.denoise_spec(0.15, 3.0, sentinel_id=SENT, segment_tokens=568, seed=1)
    s = D.spec(spec.density, spec.mean_span_q8, seed=1, seg=568, sent=SENT)
    kw = dict(pad_id=0, eos_id=1)
    dev_s, host_s = [], []
    for i in range(1 + args.reps):
        t = time.perf_counter()
        got = tok.encode_batch_denoise(docs, 512, 114, spec, decoder_start_id=0, **kw)
        dev_s.append(time.perf_counter() - t)
    for i in range(1 + min(args.reps, 2)):
        t = time.perf_counter()
        tokens = [x.tolist() for x in tok.encode_batch(docs)]
        t1 = time.perf_counter()
        ins, tgs, unit_doc = D.ref_apply(tokens, s)
        t2 = time.perf_counter()
        fi, oi = D.flat(ins)
        ft, ot = D.flat(tgs)
        enc = mbpe.pack_tokens(fi, oi, 512, **kw)
        dec = mbpe.pack_tokens_aux(ft, ot, 114, bos_id=0, labels=True, **kw)
        t3 = time.perf_counter()
        host_s.append({"total": t3 - t, "encode": t1 - t, "rule": t2 - t1, "packs": t3 - t2})
    assert np.array_equal(got["enc_ids"], enc[0]) and np.array_equal(got["dec_ids"], dec["ids"])
    assert np.array_equal(got["dec_labels"], dec["labels"]) and got["row_doc"].tolist() == unit_doc
    host = host_s[1:]
    print(json.dumps({
        "step": "tokenizer", "lib": mbpe.lib().mbpe_version().decode(), "documents": len(docs), "rows": len(unit_doc),
        "text_bytes": sum(len(d) for d in docs), "tokens": tok.n_tokens, "device_route_s": spread(dev_s[1:]),
        "host_route_s": spread([h["total"] for h in host]), "host_route_parts_s": host[-1],
        "ratio_host_to_device": statistics.median([h["total"] for h in host]) / statistics.median(dev_s[1:])}))
    tok.close()


def step_aux(args):
    import numpy as np
    import torch
    import mbpe
    import oracle as O
    dev = torch.device("cuda", 0)
    sh = open(SHAKESPEARE, "rb").read()
    merges = O.parse_model(open(MODEL, "rb").read())[2]
    pattern = mbpe.split_pattern("gpt4")
    parts, first, at = [], [0], 0
    for x in sh.splitlines(keepends=True):                           # every line split on its own
        o = mbpe.presplit(pattern, x)
        parts.append(o[1:] + np.uint64(at))
        at += len(x)
        first.append(first[-1] + len(o) - 1)
    one_off, one_doc = np.concatenate([[0]] + parts).astype(np.uint64), np.array(first, dtype=np.uint64)
    rep = args.rep
    off = np.concatenate([[0]] + [one_off[1:] + np.uint64(r * len(sh)) for r in range(rep)]).astype(np.uint64)
    docs = np.concatenate([[0]] + [one_doc[1:] + np.uint64(r * (len(one_off) - 1)) for r in range(rep)]).astype(np.uint64)
    text = torch.from_numpy(np.frombuffer(sh, dtype=np.uint8).copy()).to(dev).repeat(rep)
    torch.cuda.synchronize()
    src = dict(text_ptr=text.data_ptr(), n_bytes=text.numel())
    res = {"step": "aux", "device": torch.cuda.get_device_name(0), "lib": mbpe.lib().mbpe_version().decode(), "rep": rep,
           "text_bytes": text.numel(), "documents": len(docs) - 1, "calls": {}}
    kw = dict(seq_len=2048, layout="packed")
    with mbpe.Encoder(merges) as enc:
        for name, fim in (("aux", None), ("aux fim", mbpe.fim_spec(0.5, 0.5, 60001, 60002, 60003, seed=1))):
            enc.set_fim(fim)
            n_rows = len(enc.encode_batch_aux(None, off, docs, **kw, **src)["ids"])
            d_ids, d_lab, d_pos, d_seg = (torch.empty((n_rows, 2048), dtype=torch.int32, device=dev) for _ in range(4))
            d_len = torch.empty(n_rows, dtype=torch.int32, device=dev)
            out = dict(out_ptr=d_ids.data_ptr(), len_ptr=d_len.data_ptr(), cap_rows=n_rows, labels_ptr=d_lab.data_ptr(),
                       pos_ptr=d_pos.data_ptr(), seg_ptr=d_seg.data_ptr())
            torch.cuda.synchronize()
            total, pack = [], []
            for i in range(1 + args.reps):
                assert enc.encode_batch_aux(None, off, docs, **kw, **src, **out) == n_rows
                if i:
                    total.append(enc.kernel_ms()); pack.append(enc.pack_ms())
            res["calls"][name] = {"rows": n_rows, "tokens": enc.n_tokens, "kernel_ms": spread(total), "pack_ms": spread(pack)}
    print(json.dumps(res))


STEPS = {"stage": step_stage, "tokenizer": step_tokenizer, "aux": step_aux}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--step", choices=sorted(STEPS))
    ap.add_argument("--workload", choices=["short", "long"], default="short")
    ap.add_argument("--rep", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json")
    ap.add_argument("--timeout", type=int, default=240)
    args = ap.parse_args()
    if args.step:
        STEPS[args.step](args)
        return 0
    plan = [("stage", ["--workload", "short"]), ("stage", ["--workload", "long"]), ("tokenizer", ["--rep", "1"]), ("aux", [])]
    results = []
    for step, extra in plan:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--rep", str(args.rep), "--reps", str(args.reps)]
        try:
            r = subprocess.run(cmd + extra, capture_output=True, text=True, timeout=args.timeout)
        except subprocess.TimeoutExpired:
            print("step %s ran into its time limit" % step, file=sys.stderr)
            break
        if r.returncode != 0:
            print("step %s failed (%d):\n%s" % (step, r.returncode, r.stderr[-3000:]), file=sys.stderr)
            break
        row = json.loads(r.stdout.strip().splitlines()[-1])
        results.append(row)
        print(json.dumps(row))
        sys.stdout.flush()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)
    return 0 if len(results) == len(plan) else 1


if __name__ == "__main__":
    sys.exit(main())
