"""The token frequency tables without a GPU: the host restatements of csrc/hist.h (hist_host, hist_runs_host, the fold)
against a std::map count, as a stand-alone program (plain and under ASan + UBSan); the Python shapes of
tests/hist_cases.py against themselves; and that the library declares what the binding names."""
import os
import subprocess

import numpy as np
import pytest

import hist_cases as H

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "minbpe-cc_amd", "csrc")

FLAGS = {
    "plain": ["-O2"],
    "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
}


@pytest.mark.parametrize("build", sorted(FLAGS))
def test_hist_host_restatement(build, tmp_path):
    exe = str(tmp_path / "hist_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Wextra", "-Werror"] + FLAGS[build] +
                          ["-I" + CSRC, os.path.join(HERE, "hist_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.strip().endswith("0 failures")


def test_shapes_are_what_they_say():
    assert len(H.EDGE_IDS) == 3 * 17 and min(H.EDGE_IDS) == 255 and max(H.EDGE_IDS) == (1 << 24) + 1
    t = H.edge_tokens(4097)
    assert set(H.EDGE_IDS) <= set(t.tolist()) and int(t.max()) <= H.MAX_COUNT_IDS + 1
    counts, other = H.reference(t, 257)
    assert int(counts.sum()) + other == len(t) and counts[255] >= 1 and counts[256] >= 1
    z = H.zipf_tokens(1 << 16, 1 << 24)
    assert np.count_nonzero(z < 256) > len(z) // 4 and int(z.max()) < (1 << 24)
    f = H.flagged(t)
    assert np.array_equal(f & np.uint32(0x7FFFFFFF), t) and (f[::3] >> 31).all()


def test_symbols_are_declared():
    import mbpe
    L = mbpe.lib()
    for s in ("mbpe_token_counts", "mbpe_encoder_count", "mbpe_encoder_count_endmask", "mbpe_encoder_counts",
              "mbpe_encoder_counts_reset"):
        assert s in mbpe.EXPORTS and getattr(L, s).argtypes, s
    for s in ("mbpe_tok_count_tokens", "mbpe_tok_token_counts", "mbpe_tok_token_counts_reset"):
        assert s in mbpe.TOK_EXPORTS and getattr(L, s).argtypes, s
