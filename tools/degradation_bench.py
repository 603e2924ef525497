"""Duration of predict_bwe's known degradations on the GPU (csrc/degrade.hip, csrc/resample_sinc.hip) next to the FIR
(babe_fir_same, 500 taps) at the benchmark's shape, B = 2 segments of 368368 samples at 44.1 kHz:
  * forward + adjoint of the IIR filter (cheby1, ripple 0.05, fc 3 kHz, orders 2 / 6 / 8), the resampler (fs 4 kHz) and the
    decimation (factor 2): one of each = the degradation work of ONE score evaluation;
  * --sampler: a full-width predict_bwe('cheby1', order 6) against predict_bwe('firwin') at T = 35 on the same box.
Device-event timing.  For kernel times run the op part alone under rocprofv3 --kernel-trace --stats (--ops-only).

    python tools/degradation_bench.py [--ops-only] [--sampler]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FS, L, B = 44100, 368368, 2


def timed(fn, n=50, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3          # us per call


def ops():
    from babe_amd.degrade import DecimateDegradation, IIRDegradation, ResampleDegradation
    from babe_amd.stft import fir_same
    from babe_amd.utils.bandwidth_extension import get_cheby1_ba, get_FIR_lowpass
    g = torch.Generator().manual_seed(0)
    x = (0.1 * torch.randn(B, L, generator=g)).cuda()
    res = {}
    taps = get_FIR_lowpass(500, 3000, 1, FS).reshape(-1).cuda()
    res["fir500_fwd_adj_us"] = timed(lambda: fir_same(fir_same(x, taps), taps, adjoint=True))
    for order in (2, 6, 8):
        A = IIRDegradation(*get_cheby1_ba(order, 0.05, 2 * 3000 / FS), clamp=False, device="cuda")
        res[f"cheby1_o{order}_fwd_adj_us"] = timed(lambda: A.adj(A.fwd(x)))
        res[f"cheby1_o{order}_fwd_us"] = timed(lambda: A.fwd(x))
    A = ResampleDegradation(FS / 4000, L)
    res["resample_fs4000_fwd_adj_us"] = timed(lambda: A.adj(A.fwd(x)))
    A = DecimateDegradation(2, L)
    res["decimate2_fwd_adj_us"] = timed(lambda: A.adj(A.fwd(x)))
    return res


def sampler(T=35):
    from babe_amd.config import default_args
    from babe_amd.diff_params.edm import EDM
    from babe_amd.networks.cqtdiff_plus import Unet_CQT_oct_with_attention, init_state_dict
    from babe_amd.testing.blind_bwe_sampler import BlindSampler
    from babe_amd.utils.bandwidth_extension import apply_low_pass, get_cheby1_ba, get_FIR_lowpass
    args = default_args(sample_rate=FS, audio_len=L, T=T)
    net = Unet_CQT_oct_with_attention(args, "cuda")
    net.load_state_dict(init_state_dict(args.network.Ns, args.network.num_dils, seed=0, gate_scale=1.0))
    smp = BlindSampler(net, EDM(args), args)
    g = torch.Generator().manual_seed(1)
    clean = (0.1 * torch.randn(B, L, generator=g)).cuda()
    filts = {"firwin": get_FIR_lowpass(500, 3000, 1, FS), "cheby1": get_cheby1_ba(6, 0.05, 2 * 3000 / FS)}
    ys = {k: apply_low_pass(clean, f, k).contiguous() for k, f in filts.items()}
    out = {}
    for k in ("firwin", "cheby1"):
        smp.predict_bwe(ys[k], filts[k], k)                         # warm-up
    torch.cuda.synchronize()
    for rep in range(2):
        for k in ("firwin", "cheby1"):                              # alternated on the same box
            torch.manual_seed(3)
            t0 = time.perf_counter()
            smp.predict_bwe(ys[k], filts[k], k)
            torch.cuda.synchronize()
            out.setdefault(f"predict_bwe_{k}_T{T}_s", []).append(time.perf_counter() - t0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ops-only", action="store_true")
    ap.add_argument("--sampler", action="store_true")
    a = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    res = {"B": B, "L": L, "fs": FS}
    res.update(ops())
    if a.sampler and not a.ops_only:
        res.update(sampler())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
