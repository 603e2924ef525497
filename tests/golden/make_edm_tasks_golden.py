"""Generate tests/golden/edm_sampler_tasks.npz by IMPORTING the reference (build container only):
    python tests/golden/make_edm_tasks_golden.py [--spread]

Declipping, compressed sensing and phase retrieval posed to the reference's BASE testing.edm_sampler.Sampler(model, diff_params,
args, rid=True): its task subclasses (SamplerDeclipping, SamplerCompSens, SamplerPhaseRetrieval, :308-384) pass seven arguments to
a four-argument constructor and cannot be built.  predict_conditional(y, degradation) runs declipping and compressed sensing,
predict_resample(y, (B, audio_len), degradation) phase retrieval; the three degradations are stated here: torch.clip, a mask
product, and the magnitude of a torch.stft of the signal extended by win zeros (periodic Hamming window, center=False).  The
phase-retrieval observation is 3-D, so the reference's torch.linalg.norm(y - A(x), dim=(1, 2), ord=2) is the MATRIX 2-norm there.

Setup of make_golden.py's edm_sampler_inpainting.npz: reduced-width weights of unet_small.npz, residual wrapper a = 0.3, tester
config edm_DC_correction_4s.yaml (xi = 0.25, no data consistency), 22.05 kHz, L = 92092, T = 3, B = 1, noises recorded by replacing
torch.randn for the call.  92092 % 256 = 188: no frame of the phase-retrieval case lies wholly in the padding (the reference's
sqrt has a NaN gradient at an all-zero frame).  Every observation follows from the seed (signals() below; the tests rebuild them
the same way), so none is stored.  Per task: the final x at every 2nd sample (three full float32 signals would pass the size limit
of a committed file), t, and the state after every step at every 16th sample.

--spread: instead of writing the fixture, run phase retrieval twice more, with a float64 network and with the float32 one, and
print the difference of the two trajectories: the reference's own float32 spread, the yardstick for that task's bar.
"""
import contextlib
import importlib
import io
import os
import sys

import numpy as np
import torch
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402  (installs the reference shim; small_args, build_ref_net, ResidualNetRef, save)

SEED, RES_A, WIN, HOP, STRIDE, X_STRIDE = 2727, 0.3, 1024, 256, 16, 2
KEEP = 0.05                     # compressed sensing: fraction of samples kept
CLIP = 0.08                     # declipping: |clean| ~ 0.1 N(0, 1), so P(|clean| > 0.08) = 42 %


def setup(dtype=torch.float32):
    esm = importlib.import_module("testing.edm_sampler")
    args = mg.small_args(T=3)
    with open(f"{mg.ref_shim.REF}/conf/tester/edm_DC_correction_4s.yaml") as f:
        args.tester = mg.ref_shim.to_attr(yaml.safe_load(f))
    args.tester.T = 3
    net, _ = mg.build_ref_net(args)
    if dtype == torch.float64:
        net = net.double()
    with mg.quiet():
        s = esm.Sampler(mg.ResidualNetRef(net, RES_A, 0.063), mg.edm_mod.EDM(args), args, rid=True)
    return args, s


def signals(L):
    g = torch.Generator().manual_seed(SEED)
    clean = 0.1 * torch.randn(1, L, generator=g)
    noises = [torch.randn(1, L, generator=g) for _ in range(1 + 3)]
    mask = (torch.rand(1, L, generator=g) < KEEP).float()
    return clean, noises, mask


def stft_mag(x):
    xp = torch.cat((x, torch.zeros(x.shape[0], WIN, dtype=x.dtype)), -1)
    X = torch.stft(xp, WIN, hop_length=HOP, window=torch.hamming_window(WIN, dtype=x.dtype), center=False, return_complex=True)
    return torch.sqrt(X.real ** 2 + X.imag ** 2)


def run(call, noises, dtype=torch.float32):
    it = iter(noises)
    orig = torch.randn
    torch.randn = lambda *a, **k: next(it).to(dtype)
    try:
        with mg.quiet(), contextlib.redirect_stderr(io.StringIO()):
            x, den, t = call()
    finally:
        torch.randn = orig
    return x[..., ::X_STRIDE], den[..., ::STRIDE], t


def spread():
    outs = []
    for dtype in (torch.float64, torch.float32):
        args, s = setup(dtype)
        L = args.exp.audio_len
        clean, noises, _ = signals(L)
        y = stft_mag(clean).to(dtype)
        if dtype == torch.float64:
            torch.set_default_dtype(torch.float64)               # (the schedule and the prior sample follow the network)
        try:
            outs.append(run(lambda: s.predict_resample(y, (1, L), stft_mag), noises, dtype))
        finally:
            torch.set_default_dtype(torch.float32)
    (x64, d64, _), (x32, d32, _) = outs
    rms = lambda a, b: float((a.double() - b.double()).pow(2).mean().sqrt())
    rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())
    print(f"phase retrieval, reference float32 against float64: final x rms {rms(x32, x64):.3e} rel {rel(x32, x64):.3e}; "
          f"per-step states rms {rms(d32, d64):.3e} rel {rel(d32, d64):.3e}")


def main():
    args, s = setup()
    L = args.exp.audio_len
    clean, noises, mask = signals(L)
    out = dict(seed=SEED, res_a=RES_A, stride=STRIDE, x_stride=X_STRIDE, xi=args.tester.posterior_sampling.xi, ro=args.tester.diff_params.ro,
               sigma_max=args.tester.diff_params.sigma_max, Schurn=args.tester.diff_params.Schurn, clip_value=CLIP,
               keep=KEEP, win=WIN, hop=HOP)

    y = torch.clip(clean, -CLIP, CLIP)
    clipped = float((clean.abs() > CLIP).float().mean())
    assert 0.05 <= clipped <= 0.50, clipped
    x, den, t = run(lambda: s.predict_conditional(y.clone(), lambda v: torch.clip(v, -CLIP, CLIP)), noises)
    out.update(declip_clipped=clipped, declip_x=x, declip_den=den, t=t)

    assert abs(float(mask.mean()) - KEEP) < 0.005
    x, den, t2 = run(lambda: s.predict_conditional((mask * clean).clone(), lambda v: mask * v), noises)
    assert torch.equal(t, t2)
    out.update(compsens_x=x, compsens_den=den)

    y = stft_mag(clean)
    assert y.shape == (1, WIN // 2 + 1, 1 + L // HOP) and L % HOP != 0
    x, den, t3 = run(lambda: s.predict_resample(y.clone(), (1, L), stft_mag), noises)
    assert torch.equal(t, t3) and bool(torch.isfinite(x).all())
    out.update(pr_x=x, pr_den=den)
    mg.save("edm_sampler_tasks.npz", **out)


if __name__ == "__main__":
    spread() if "--spread" in sys.argv else main()
