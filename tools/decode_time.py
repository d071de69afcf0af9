"""Decode on the device (csrc/decode.hip) timed: kernel time, output rate, share of the bandwidth peak on the byte count
of DESIGN 4e, and two comparisons taken in the same process --

  * the host Tokenizer::decode (mbpe_tok_decode) of the same tokens against the device path INCLUDING both copies
    (mbpe_decode_tokens, host tokens in, host bytes out), over a range of sizes, with the crossover;
  * a device-to-device copy of as many bytes as the output: the copy moves 2 x output, decode (4 or 2 B x tokens x 2 +
    output), so copy time x that ratio is the floor of the decode.

Workloads: shakespeare.txt x N encoded with the shakespeare gpt4 model (32-bit ids), and the final 16-bit slot stream
of a one-chunk SplitMix64 training (config-4 style).  Kernel time = HIP events on the decoder's stream around its
three kernels (mbpe_decoder_kernel_ms), warm, median of --reps.

    python tools/decode_time.py [--json out.json] [--quick]       (from the repository root, on a GPU)
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/decode_time.py --quick      (a run of its own)
"""
import argparse
import ctypes
import json
import statistics
import sys
import time

sys.path[:0] = ["tests", "oracle", "minbpe-cc_amd/python"]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import mbpe  # noqa: E402
import oracle as O  # noqa: E402

PEAK_BYTES_PER_S = 8e12


def wall(f, reps):
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t)
    return statistics.median(ts)


def copy_ms(n_bytes, dev, reps):
    """Device-to-device copy of n_bytes, torch events, warm, median."""
    src = torch.empty(n_bytes, dtype=torch.uint8, device=dev)
    dst = torch.empty(n_bytes, dtype=torch.uint8, device=dev)
    src.fill_(7)
    for _ in range(3):
        dst.copy_(src)
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        dst.copy_(src)
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def device_case(name, run, n_tokens, token_bytes, n_out, dev, reps):
    for _ in range(3):
        run()
    ms = []
    for _ in range(reps):
        ms.append(run())
    k = statistics.median(ms)
    moved = 2 * token_bytes * n_tokens + n_out
    c = copy_ms(n_out, dev, reps)
    floor = c * moved / (2 * n_out)
    return {"case": name, "n_tokens": n_tokens, "token_bytes": token_bytes, "out_bytes": n_out,
            "kernel_ms_median": k, "kernel_ms_min": min(ms), "kernel_ms_max": max(ms), "reps": reps,
            "out_GBps": n_out / k / 1e6, "bytes_moved": moved, "share_of_8TBps": moved / (k * 1e-3) / PEAK_BYTES_PER_S,
            "d2d_copy_ms": c, "floor_ms": floor, "multiple_of_floor": k / floor}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quick", action="store_true", help="device timing of shakespeare x 64 only (for a kernel trace)")
    ap.add_argument("--train-mib", type=int, default=1024)
    ap.add_argument("--train-vocab", type=int, default=32000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("decode_time.py needs a GPU: there is nothing to time without one")
    dev = torch.device("cuda", 0)
    L = mbpe.lib()
    sh = open("tests/golden/data/shakespeare.txt", "rb").read()
    merges = O.parse_model(open("tests/golden/shakespeare_gpt4_lexical_512.model", "rb").read())[2]
    tok = mbpe.Tokenizer(O.GPT4_SPLIT_PATTERN)
    tok.set_merges(merges)
    enc1 = np.ascontiguousarray(tok.encode(sh, device=0), dtype=np.uint32)      # chunks never interact: x N = tiled
    res = {"device": torch.cuda.get_device_name(0), "shakespeare_bytes": len(sh), "shakespeare_tokens": len(enc1),
           "device_cases": [], "host_vs_device": []}
    dec = mbpe.Decoder(merges)

    for rep in ((64,) if args.quick else (64, 1024)):
        t = torch.from_numpy(np.tile(enc1, rep).view(np.int32)).to(dev)
        n_out = len(sh) * rep
        out = torch.empty(n_out, dtype=torch.uint8, device=dev)

        def run():
            assert dec.decode_device(t.data_ptr(), t.numel(), out.data_ptr(), n_out) == (n_out, 0)
            return dec.kernel_ms()
        res["device_cases"].append(device_case("shakespeare_x%d" % rep, run, t.numel(), 4, n_out, dev, args.reps))
        want = torch.from_numpy(np.frombuffer(sh, dtype=np.uint8).copy()).to(dev)
        assert bool((out.view(rep, len(sh)) == want).all())
        del t, out
    if args.quick:
        print(json.dumps(res))
        return

    # host Tokenizer::decode against the device path with both copies
    n, bad = ctypes.c_uint64(), ctypes.c_uint64()
    for rep in (1, 4, 16, 64, 256, 1024):
        t = np.tile(enc1, rep)
        n_out = len(sh) * rep
        buf = np.zeros(n_out, dtype=np.uint8)
        reps = 5 if rep <= 64 else (3 if rep <= 256 else 1)

        def host():
            assert L.mbpe_tok_decode(tok._h, t.ctypes.data, len(t), 0, buf.ctypes.data, n_out, ctypes.byref(n)) == 0

        def device():
            assert L.mbpe_decode_tokens(dec._h, t.ctypes.data, len(t), 0, buf.ctypes.data, n_out, 0, ctypes.byref(n),
                                        ctypes.byref(bad)) == 0

        def device_tok():
            assert L.mbpe_tok_decode_device(tok._h, t.ctypes.data, len(t), 0, 0, buf.ctypes.data, n_out, ctypes.byref(n)) == 0
        device()
        device_tok()                                               # warm: decoder of the tokenizer, staging buffers
        h = wall(host, reps)
        assert n.value == n_out and buf[:len(sh)].tobytes() == sh and buf[-len(sh):].tobytes() == sh
        buf[:] = 0
        d = wall(device, max(reps, 3))
        assert n.value == n_out and buf[:len(sh)].tobytes() == sh and buf[-len(sh):].tobytes() == sh
        dt = wall(device_tok, max(reps, 3))
        res["host_vs_device"].append({"x": rep, "n_tokens": len(t), "out_bytes": n_out, "host_decode_s": h,
                                      "device_with_copies_s": d, "tokenizer_device_decode_s": dt,
                                      "host_GBps": n_out / h / 1e9, "device_with_copies_GBps": n_out / d / 1e9,
                                      "device_faster": d < h})
    faster = [r["device_faster"] for r in res["host_vs_device"]]
    cross = None
    for i, r in enumerate(res["host_vs_device"]):
        if all(faster[i:]):
            cross = r["x"]
            break
    res["crossover_x"] = cross
    res["pass_device_faster_at_x1024"] = res["host_vs_device"][-1]["device_faster"]
    dec.close()

    # the final stream of a one-chunk training (16-bit slots, holes included)
    data = O.splitmix64_bytes(42, args.train_mib << 20)
    with mbpe.Trainer(0) as tr:
        tr.load_corpus(data)
        tr.train_begin(args.train_vocab)
        tr.train_steps(args.train_vocab - 256)
        m = tr.train_result()[0]
        ptr, n_slots, bits, end_bit, barrier = tr.stream_device()
        st = tr.stats()
        out = torch.empty(len(data), dtype=torch.uint8, device=dev)
        with mbpe.Decoder(m) as d2:
            def run():
                assert d2.decode_slots_device(ptr, n_slots, bits, end_bit, barrier, out.data_ptr(), len(data)) == (len(data), 0)
                return d2.kernel_ms()
            case = device_case("splitmix64_%dMiB_vocab%d_final_stream" % (args.train_mib, args.train_vocab), run, n_slots,
                               bits // 8, len(data), dev, args.reps)
        case["n_live"] = st["n_live"]
        case["merges"] = len(m)
        res["device_cases"].append(case)
        step = 1 << 26
        for lo in range(0, len(data), step):
            assert bool(torch.equal(out[lo:lo + step].cpu(), torch.from_numpy(data[lo:lo + step]))), lo
    print(json.dumps(res))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
