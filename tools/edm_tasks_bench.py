"""Duration of the declipping and phase-retrieval operators on the GPU (csrc/edm_tasks.hip) at the benchmark's shape, B = 2 segments
of 368368 samples at 44.1 kHz, next to the FIR pair (babe_fir_same, 500 taps):
  * the fused clip residual + masked adjoint, and forward + VJP of the STFT magnitude at (win, hop) = (1024, 256), each split into
    its halves, and the matrix-2-norm seed of phase retrieval: the degradation work of ONE score evaluation;
  * --sampler: a full-width predict_pr and predict_declipping against predict_bwe('firwin') at T = 35 on the same box.
Device-event timing.  For kernel times run the op part alone under rocprofv3 --kernel-trace --stats (--ops-only).

    python tools/edm_tasks_bench.py [--ops-only] [--sampler]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.degradation_bench import timed  # noqa: E402

FS, L, B = 44100, 368368, 2
WIN, HOP, CLIP = 1024, 256, 0.08


def ops():
    from babe_amd.degrade import ClipDegradation, STFTMagnitudeDegradation, specnorm_seed
    from babe_amd.stft import fir_same
    from babe_amd.utils.bandwidth_extension import get_FIR_lowpass
    g = torch.Generator().manual_seed(0)
    x = (0.1 * torch.randn(B, L, generator=g)).cuda()
    res = {}
    taps = get_FIR_lowpass(500, 3000, 1, FS).reshape(-1).cuda()
    res["fir500_fwd_adj_us"] = timed(lambda: fir_same(fir_same(x, taps), taps, adjoint=True))
    A = ClipDegradation(CLIP)
    y = A.fwd(x)
    res["clip_residual_adj_us"] = timed(lambda: A.adj(A.residual(x, y)[0]))
    res["clip_residual_us"] = timed(lambda: A.residual(x, y))
    A = STFTMagnitudeDegradation(WIN, HOP, L, "cuda")
    gm = torch.randn(B, A.bins * A.frames, generator=g).cuda()
    res["stft_mag_fwd_vjp_us"] = timed(lambda: A.adj(A.fwd(x)))
    res["stft_mag_fwd_us"] = timed(lambda: A.fwd(x))
    res["stft_mag_vjp_us"] = timed(lambda: A.adj(gm))
    res["specnorm_seed_us"] = timed(lambda: specnorm_seed(gm, A.bins, A.frames))          # 32 power iterations, 66 launches
    return res


def sampler(T=35):
    from babe_amd.config import default_args
    from babe_amd.degrade import STFTMagnitudeDegradation
    from babe_amd.diff_params.edm import EDM
    from babe_amd.networks.cqtdiff_plus import Unet_CQT_oct_with_attention, init_state_dict
    from babe_amd.testing.edm_sampler import Sampler
    from babe_amd.utils.bandwidth_extension import apply_low_pass, get_FIR_lowpass
    args = default_args(sample_rate=FS, audio_len=L, T=T)
    net = Unet_CQT_oct_with_attention(args, "cuda")
    net.load_state_dict(init_state_dict(args.network.Ns, args.network.num_dils, seed=0, gate_scale=1.0))
    smp = Sampler(net, EDM(args), args)
    g = torch.Generator().manual_seed(1)
    clean = (0.1 * torch.randn(B, L, generator=g)).cuda()
    taps = get_FIR_lowpass(500, 3000, 1, FS)
    ylpf = apply_low_pass(clean, taps, "firwin").contiguous()
    ymag = STFTMagnitudeDegradation(WIN, HOP, L, "cuda").fwd(clean)
    yclip = torch.clip(clean, -CLIP, CLIP)
    runs = {"bwe_firwin": lambda: smp.predict_bwe(ylpf, taps, "firwin"),
            "declipping": lambda: smp.predict_declipping(yclip, CLIP),
            "pr": lambda: smp.predict_pr(ymag, WIN, HOP)}
    out = {}
    runs["bwe_firwin"]()                                            # warm-up
    torch.cuda.synchronize()
    for rep in range(2):
        for k, fn in runs.items():                                  # alternated on the same box
            torch.manual_seed(3)
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.setdefault(f"predict_{k}_T{T}_s", []).append(time.perf_counter() - t0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ops-only", action="store_true")
    ap.add_argument("--sampler", action="store_true")
    a = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    res = {"B": B, "L": L, "fs": FS, "win": WIN, "hop": HOP}
    res.update(ops())
    if a.sampler and not a.ops_only:
        res.update(sampler())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
