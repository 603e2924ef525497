"""The tail of the A-weighted training loss at a training batch's shape, B = 4 segments of 368368 samples, 101 taps: the fused
kernels (stft.fir_sqerr: babe_fir_sqerr_fwd / _bwd, csrc/loss.hip) against the chain they replace, built from the ops that were
there before - torch sub -> babe_fir_same -> torch square forward, autograd's 2 * ew * g -> babe_fir_same(adjoint) backward.  Each
variant is timed forward + backward with device events over N calls after a warm-up, the two alternated REPS times on the same
box; the outputs are compared first.

    python tools/aweighting_bench.py [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.degradation_bench import timed  # noqa: E402

FS, L, B, K = 44100, 368368, 4, 101
N, REPS = 2000, 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    from babe_amd.stft import fir_same, fir_sqerr
    from babe_amd.utils.training_utils import FIRFilter
    gen = torch.Generator().manual_seed(0)
    est, tgt, g = (torch.randn(B, L, generator=gen).cuda() for _ in range(3))
    taps = FIRFilter("aw", fs=FS, ntaps=K).taps.cuda()

    def fused():
        x = est.detach().requires_grad_(True)
        err2 = fir_sqerr(x, tgt, taps)
        return err2, torch.autograd.grad(err2, x, grad_outputs=g)[0]

    def chain():
        ew = fir_same(est - tgt, taps)
        err2 = ew * ew
        return err2, fir_same(2 * ew * g, taps, adjoint=True)

    (e_f, g_f), (e_c, g_c) = fused(), chain()
    res = {"B": B, "L": L, "K": K, "calls": N,
           "err2_maxdiff_rel": float((e_f - e_c).abs().max() / e_c.abs().max()),
           "grad_maxdiff_rel": float((g_f - g_c).abs().max() / g_c.abs().max()), "fused_fwd_bwd_us": [], "chain_fwd_bwd_us": []}
    for _ in range(REPS):
        res["fused_fwd_bwd_us"].append(round(timed(fused, n=N, warm=20), 2))
        res["chain_fwd_bwd_us"].append(round(timed(chain, n=N, warm=20), 2))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
