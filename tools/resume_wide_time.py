"""The direct begin of a training continued from existing merges on 32-bit tokens (mbpe_train_begin_from with
"resume_wide" 1 and n_prior at or past the handover; csrc/wide.hip: k_wide_pair_count_tokens), timed on two corpora:

    shakespeare   shakespeare.txt x 1024, gpt4 split on the device, 256 prior merges, "wide_from" 0 -- the stream of
                  profiles/r15_resume.md, whose 16-bit count kernel took 16.7 ms
    words         4,200 random words x 24 bytes, one chunk per occurrence, 66,000 - 256 prior merges (17-bit ids)

    python tools/resume_wide_time.py CASE [--json out.json] [--scale N]      (from the repository root, on a GPU)

The prior merges come from a training on the same corpus.  The resumed begin then runs twice (the second, warm one is
reported) and one merge follows, so that a kernel trace of the run holds the first argmax.  ms_begin is the device time
between the events around the begin plus the replay's; its split by kernel comes from a run of this script under
`rocprofv3 --kernel-trace --stats`.  Nothing is asserted beyond the state being sane."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "minbpe-cc_amd", "python")]
import numpy as np  # noqa: E402

import mbpe  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("case", choices=["shakespeare", "words"])
    ap.add_argument("--json")
    ap.add_argument("--scale", type=int, default=1, help="shakespeare: a corpus N times smaller (rehearsal)")
    args = ap.parse_args()
    res = {"case": args.case}
    keep = []
    if args.case == "shakespeare":
        import torch
        dev = torch.device("cuda", 0)
        with open(os.path.join(ROOT, "tests", "golden", "data", "shakespeare.txt"), "rb") as f:
            one = np.frombuffer(f.read(), dtype=np.uint8)
        text = torch.from_numpy(np.tile(one, max(1024 // args.scale, 1))).to(dev)
        sp = mbpe.Splitter(mbpe.split_pattern("gpt4"))
        res["n_chunks"] = sp.split(offsets=False, text_ptr=text.data_ptr(), n_bytes=text.numel())
        mask_ptr, _, _ = sp.endmask()
        keep.append(sp)
        n_prior, vocab, n_bytes = 256, 768, int(text.numel())

        def load(tr):
            tr.load_corpus_endmask(mask_ptr, text_ptr=text.data_ptr(), n_bytes=text.numel(), keep=text)
    else:
        from test_gpu_wide import _word_corpus
        data, off = _word_corpus(78, 4200, 24, (6, 14))
        n_prior, vocab, n_bytes = 66000 - 256, 68000, len(data)

        def load(tr):
            tr.load_corpus(data, off)
    res.update(n_bytes=n_bytes, n_prior=n_prior, vocab=vocab)

    with mbpe.Trainer(0) as tr:
        load(tr)
        tr.train_begin(256 + n_prior)
        assert tr.train_steps(n_prior) == n_prior
        st = tr.stats()
        res["train"] = {"ms_begin": st["ms_begin"], "ms_steps": st["ms_steps"], "n_live_after": st["n_live"]}
        prior, _ = tr.train_result()
        tr.set_option("resume_wide", 1)
        tr.set_option("wide_from", 0)
        for run in ("cold", "warm"):
            load(tr)
            tr.train_begin(vocab, prior_merges=prior)
            st = tr.stats()
            assert tr.stream_device()[2] == 32 and st["n_merges"] == n_prior
            res["begin_%s" % run] = {"ms_begin": st["ms_begin"], "n_tokens": st["n_live"], "n_pairs": st["n_pairs"]}
            print(run, res["begin_%s" % run], flush=True)
        assert st["n_live"] == res["train"]["n_live_after"]
        res["merges_after"] = tr.train_steps(1)
        res["ms_first_merge"] = tr.stats()["ms_steps"]
    print(json.dumps(res, sort_keys=True))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
