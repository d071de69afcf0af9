"""Measurements behind profiles/r15_resume.md: what mbpe_train_begin_from costs against reaching the same state by
training (mbpe_train_begin + the first n_prior merges), on the two workloads the note names.

  python profiles/collect_r15.py shakespeare OUT.json     shakespeare.txt x 1024, gpt4 split on the device, 256 -> 768
  python profiles/collect_r15.py splitmix OUT.json        1 GiB of SplitMix64 (seed 42), one chunk, 1,024 -> 2,048
  ... --begin-only PRIOR.npy                              only the resumed begin, twice (for a kernel trace: run this
                                                          under `rocprofv3 --kernel-trace --stats`; the second begin
                                                          is the warm one)
  ... --scale N                                           rehearsal: a corpus N times smaller

Times are device times from mbpe_stats (HIP events on the context's stream; ms_begin of a resumed begin includes the
encoder's).  Every number is printed and written to OUT.json; nothing is asserted."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "minbpe-cc_amd", "python"))
sys.path.insert(0, ROOT)

import mbpe  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("case", choices=["shakespeare", "splitmix"])
    ap.add_argument("out")
    ap.add_argument("--begin-only", metavar="PRIOR.npy")
    ap.add_argument("--scale", type=int, default=1)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    res = {"case": args.case, "scale": args.scale}

    keep = []
    if args.case == "shakespeare":
        with open(os.path.join(ROOT, "tests", "golden", "data", "shakespeare.txt"), "rb") as f:
            one = np.frombuffer(f.read(), dtype=np.uint8)
        text = torch.from_numpy(np.tile(one, max(1024 // args.scale, 1))).to(dev)
        n_prior, vocab = 256, 768
        sp = mbpe.Splitter(mbpe.split_pattern("gpt4"))
        res["n_chunks"] = sp.split(offsets=False, text_ptr=text.data_ptr(), n_bytes=text.numel())
        mask_ptr, _, _ = sp.endmask()
        keep.append(sp)

        def load(tr):
            tr.load_corpus_endmask(mask_ptr, text_ptr=text.data_ptr(), n_bytes=text.numel(), keep=text)
    else:
        import bench
        store, text = bench.splitmix64_device(42, (1 << 30) // args.scale, dev)
        keep.append(store)
        n_prior, vocab = 1024, 2048

        def load(tr):
            tr.load_corpus_device(text.data_ptr(), text.numel(), keep=text)
    res["n_bytes"] = int(text.numel())
    res["n_prior"], res["vocab"] = n_prior, vocab

    with mbpe.Trainer(0) as tr:
        if args.begin_only:
            prior = np.load(args.begin_only)
        else:
            # what a user pays today to reach the state: begin + the first n_prior merges (second run: warm)
            for run in ("cold", "warm"):
                load(tr)
                tr.train_begin(256 + n_prior)
                st0 = tr.stats()
                done = tr.train_steps(n_prior)
                st = tr.stats()
                res["train_%s" % run] = {"ms_begin": st0["ms_begin"], "ms_steps": st["ms_steps"], "merges": done,
                                         "n_live_after": st["n_live"]}
                print(run, res["train_%s" % run], flush=True)
            prior, _ = tr.train_result()
            np.save(os.path.splitext(args.out)[0] + "_prior.npy", prior)
            # mbpe_train_begin's own ms_begin at the full vocabulary, for the record that it does not move
            load(tr)
            tr.train_begin(vocab)
            res["ms_begin_from_bytes_at_vocab"] = tr.stats()["ms_begin"]
        assert len(prior) == n_prior, len(prior)
        for table in ("dense", "hashed"):
            tr.set_option("dense_table", 1 if table == "dense" else 0)
            for run in ("cold", "warm"):
                load(tr)
                tr.train_begin(vocab, prior_merges=prior)
                st = tr.stats()
                res["resume_%s_%s" % (table, run)] = {"ms_begin": st["ms_begin"], "n_live": st["n_live"],
                                                      "n_pairs": st["n_pairs"], "n_slots": st["n_slots"]}
                print(table, run, res["resume_%s_%s" % (table, run)], flush=True)
            if args.begin_only:
                break
        if not args.begin_only:
            tr.set_option("dense_table", -1)
            more = tr.train_steps(16)
            res["merges_after_resume"] = more
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
