"""Time predict_blind_bwe with the sampling loop in Python (the default) and in the library (babe_sample_bwe, csrc/sample.hip) at
the benchmark's shape - full-width network, L = 368368, T = 35, B = 1 and B = 4 - and the noise generator (babe_randn,
csrc/randn.hip) against a plain hipMemsetAsync of the same bytes, the write-bandwidth yardstick.

    python tools/sample_c_bench.py [--T 35] [--reps 3] [--batches 1 4] [--out profiles/sample_c.txt]

Both loops run in ONE process on one GPU, alternated (python, library, python, library, ...) after one warm-up run of each and
shape; a run's time is a host clock around the call, ended by a device synchronise.  Both draw their noise from the library's
generator under one seed, so they compute the same thing (checked: bit-equal results).  No speed-up is claimed or required: the
Python loop has no launch gap to close, and at B >= 2 it runs two clip lanes where the library run is one stream (a host that
wants two runs two calls on two streams).  Needs a MI355X."""
import argparse
import ctypes
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def time_loops(args, net, B, reps, seed, lines):
    from babe_amd.diff_params.edm import EDM
    from babe_amd.testing.blind_bwe_sampler import BlindSampler
    L = args.exp.audio_len
    g = torch.Generator().manual_seed(5)
    y = (0.1 * torch.randn(B, L, generator=g)).cuda()
    smp = {"python": BlindSampler(net, EDM(args), args, loop="python", noise_device="philox", seed=seed),
           "library": BlindSampler(net, EDM(args), args, loop="library", seed=seed)}
    out, times = {}, {k: [] for k in smp}

    def run(k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        x, fp = smp[k].predict_blind_bwe(y)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, x, fp

    for k in smp:                                        # warm-up: code objects, workspaces, plans
        _, x, fp = run(k)
        out[k] = (x.clone(), fp.clone())
    assert smp["library"]._csample is not None and smp["library"]._csample.calls == 1, "the library loop did not run"
    same = torch.equal(out["python"][0], out["library"][0]) and torch.equal(out["python"][1], out["library"][1])
    for _ in range(reps):
        for k in smp:
            times[k].append(run(k)[0])
    audio = B * L / args.exp.sample_rate
    for k in smp:
        t = times[k]
        lines.append(f"predict_blind_bwe B={B} L={L} T={args.tester.T} loop={k:8s}: median {statistics.median(t):7.3f} s "
                     f"(min {min(t):.3f}, max {max(t):.3f}, {len(t)} runs) = {audio / statistics.median(t):.3f} audio-sec/s")
    lines.append(f"    results bit-equal between the loops: {same}")


def time_noise(B, L, lines, windows=11, calls=200):
    from babe_amd._lib import check, lib
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemsetAsync.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
    buf = torch.empty(B, L, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    fns = {"babe_randn": lambda: check(lib().babe_randn(buf.data_ptr(), L, B, L, 1, 0, 0, st), "randn"),
           "hipMemsetAsync": lambda: hip.hipMemsetAsync(buf.data_ptr(), 0, 4 * B * L, st)}
    res = {k: [] for k in fns}
    for f in fns.values():
        for _ in range(20):
            f()
    for _ in range(windows):
        for k, f in fns.items():                         # the two alternated, window by window
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                f()
            e1.record()
            e1.synchronize()
            res[k].append(e0.elapsed_time(e1) * 1e3 / calls)
    nbytes = 4 * B * L
    for k, v in res.items():
        us = statistics.median(v)
        lines.append(f"{k:15s} B={B} L={L} ({nbytes / 1e6:.1f} MB): median {us:8.2f} us ({min(v):.2f} .. {max(v):.2f}; {windows} windows of "
                     f"{calls} calls, HIP events) = {nbytes / us / 1e6:.3f} TB/s written")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=35)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    a = ap.parse_args()
    from babe_amd.config import default_args
    from babe_amd.networks.cqtdiff_plus import Unet_CQT_oct_with_attention, init_state_dict
    args = default_args(T=a.T)
    net = Unet_CQT_oct_with_attention(args, "cuda")
    net.load_state_dict(init_state_dict(list(args.network.Ns), args.network.num_dils, seed=0, gate_scale=1.0))
    lines = [f"device: {torch.cuda.get_device_name(0)}; one process, the two loops alternated after one warm-up run each"]
    for B in a.batches:
        time_loops(args, net, B, a.reps, a.seed, lines)
    for B in (4, 32):
        time_noise(B, args.exp.audio_len, lines)
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
