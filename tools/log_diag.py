"""Kept as the record of how profiles/r16_delta_log.md section 2 was measured, the run that decided for the delta log.
Every pass of the benchmark workload with at least LOG_DIAG_MIN pairs (default 2000) is replayed on its own: a fresh
training runs with the shipped kernel up to that pass, then the pass itself runs under every MBPE_FUSED_DIAG of
LOG_DIAG_LIST (library built with -DMBPE_DIAG; MBPE_LIB=build/libmbpe_diag.so).  The time is the pass plus whatever
follows it inside its pair of events.  In that run 0 was the kernel that counted in cell blocks, 2 the build without
count deltas, and 7 / 8 two builds that wrote log records without a consumer; 7 became the shipped kernel and both
are gone.  With today's library only 0 and 2 remain, and 0 is the shipped launch with the delta log (the DIAG
instantiations themselves hold none of the log's code)."""
import json, os, sys
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "minbpe-cc_amd", "python"))
sys.path.insert(0, ROOT)
import torch, mbpe
from bench import splitmix64_device
dev = torch.device("cuda", 0)
n, vocab = 4 << 30, 32000
min_pairs = int(os.environ.get("LOG_DIAG_MIN", "2000"))
diags = [int(x) for x in os.environ.get("LOG_DIAG_LIST", "0,2").split(",")]
keep, corpus = splitmix64_device(42, n, dev)
torch.cuda.synchronize()
tr = mbpe.Trainer(0)
tr.load_corpus_device(corpus.data_ptr(), n, keep=keep)
tr.set_option("batch", 1)
tr.set_option("time_kernels", 1)

os.environ.pop("MBPE_FUSED_DIAG", None)
tr.train_begin(vocab)
sizes, k = [], 0
while k < vocab - 256:
    got = tr.train_sequences(1)
    if got == 0:
        break
    sizes.append(got)
    k += got
picks = [i for i, g in enumerate(sizes) if g >= min_pairs]
out = {"passes": []}
for i in picks:
    row = {"sequence": i, "pairs": sizes[i], "ms_fused": {}}
    for d in diags:
        os.environ.pop("MBPE_FUSED_DIAG", None)
        tr.train_begin(vocab)
        if i:
            tr.train_sequences(i)
        s0 = tr.stats()
        os.environ["MBPE_FUSED_DIAG"] = str(d)
        try:
            tr.train_sequences(1)
        except Exception as e:              # (timing-only kernels leave wrong counts behind)
            row.setdefault("errors", []).append("diag %d: %s" % (d, e))
        s1 = tr.stats()
        row["ms_fused"][str(d)] = round(s1["ms_fused_kernel"] - s0["ms_fused_kernel"], 3)
        if d == 0:
            row["matches"] = s0["n_live"] - s1["n_live"]
    print(json.dumps(row), flush=True)
    out["passes"].append(row)
os.environ.pop("MBPE_FUSED_DIAG", None)
print(json.dumps(out))
