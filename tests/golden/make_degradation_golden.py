"""Golden vectors of predict_bwe's degradations 'cheby1', 'biquad', 'resample' and 'decimate' (the reference's
testing/blind_bwe_sampler.py:219-230, :306-364, :376-385 and utils/bandwidth_extension.py), by IMPORTING the reference:

    python tests/golden/make_degradation_golden.py

torchaudio is not installed in the build container, so a `torchaudio` stand-in goes into sys.modules before the reference is
imported (then oracle.ref_shim, through make_golden, as for the other fixtures).  It is written from torchaudio's PUBLISHED
semantics:
  * functional.lfilter(waveform, a_coeffs, b_coeffs, clamp=True): coefficients as float32, normalised by a[0] in float32; the
    filter itself applied in float64 (scipy.signal.lfilter), returned in the waveform's dtype; an autograd Function whose
    backward is the reversed filter; clamp=True clips the output to [-1, 1] with torch.clamp (and its gradient);
  * functional.biquad(waveform, b0, b1, b2, a0, a1, a2): lfilter with the six values as float32 and the default clamp=True;
  * functional.resample: oracle/resample.py's restatement of the published algorithm (imported, not edited).
The fixtures therefore pin the reference's semantics in exact (float64) recursion arithmetic, NOT torchaudio's float32
rounding of the recursion.  Data only: inputs are re-derived from the seeds stored beside them.

Writes degradation_ops_iir1k.npz / _iir3k.npz (cheby1 cases 0-2 / 3-6), degradation_ops_other.npz (operator level: A(x) and the autograd gradient of <A(x), w>, B = 2,
through the reference sampler's own apply_IIR_filter / apply_biquad / resample / decimate; prepare_filter's output; the
float32-normalised coefficients) and degradation_sampler_{cheby1,biquad,rs}.npz (the reference's predict_bwe at reduced width, T = 3, for each
type, as make_golden.py::g14; resample / decimate with start_sigma None; cheby1 once more with data_consistency on).
"""
import contextlib
import io
import os
import sys
import types

import numpy as np
import scipy.signal
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from oracle import resample as oracle_resample  # noqa: E402


def normalise_fp32(b, a):
    """What lfilter applies: float32 coefficients divided by a[0] in float32."""
    b32 = torch.as_tensor(b).float().reshape(-1)
    a32 = torch.as_tensor(a).float().reshape(-1)
    return b32 / a32[0:1], a32 / a32[0:1]


class _LFilter(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, bn, an):
        ctx.coef = (bn, an)
        y = scipy.signal.lfilter(bn, an, x.detach().double().numpy(), axis=-1)
        return torch.from_numpy(np.ascontiguousarray(y)).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        bn, an = ctx.coef
        gr = scipy.signal.lfilter(bn, an, g.detach().double().numpy()[..., ::-1], axis=-1)[..., ::-1]
        return torch.from_numpy(np.ascontiguousarray(gr)).to(g.dtype), None, None


def lfilter(waveform, a_coeffs, b_coeffs, clamp=True, batching=True):
    bn, an = normalise_fp32(b_coeffs, a_coeffs)
    y = _LFilter.apply(waveform, bn.double().numpy(), an.double().numpy())
    return torch.clamp(y, min=-1.0, max=1.0) if clamp else y


def biquad(waveform, b0, b1, b2, a0, a1, a2):
    f = lambda v: torch.as_tensor(v, dtype=waveform.dtype).view(1)      # noqa: E731
    return lfilter(waveform, torch.cat([f(a0), f(a1), f(a2)]), torch.cat([f(b0), f(b1), f(b2)]))


def resample(waveform, orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99):
    return oracle_resample.resample(waveform, orig_freq, new_freq, lowpass_filter_width, rolloff)


ta = types.ModuleType("torchaudio")
ta_f = types.ModuleType("torchaudio.functional")
ta_f.lfilter, ta_f.biquad, ta_f.resample = lfilter, biquad, resample
ta.functional = ta_f
ta.__version__ = "stand-in (published semantics, float64 recursion)"
sys.modules["torchaudio"] = ta
sys.modules["torchaudio.functional"] = ta_f

import make_golden as MG  # noqa: E402  (installs oracle.ref_shim and imports the reference)

ube = MG.importlib.import_module("utils.bandwidth_extension")
Ref = MG.samp_mod.BlindSampler

L_OPS = 12000
CHEBY = [(4, 22050, 1000), (6, 22050, 1000), (8, 22050, 1000), (4, 22050, 3000), (6, 22050, 3000), (8, 22050, 3000),
         (6, 44100, 3000)]
RIPPLE = 0.05
BIQUAD = (3000, 22050, 0.707)
RESAMPLE_FS = (2000, 4000)
DECIMATE = (2, 5)


def inputs(seed, L=L_OPS, scale=0.3):
    g = torch.Generator().manual_seed(seed)
    return scale * torch.randn(2, L, generator=g), torch.randn(2, L, generator=g)


def op_and_grad(fn, x, w_full, L_out=None):
    """A(x) and d<A(x), w>/dx (w cut to A's output length)."""
    x = x.clone().requires_grad_(True)
    y = fn(x)
    w = w_full[..., :y.shape[-1]]
    gx, = torch.autograd.grad((y * w).sum(), x)
    return y.detach(), gx


def tester_args(ftype, fc=3000, order=6, Q=0.707, fs=2000, factor=1):
    args = MG.small_args()
    bwe = args.tester.bandwidth_extension
    bwe.filter.type, bwe.filter.fc, bwe.filter.order = ftype, fc, order
    bwe.filter.biquad.Q, bwe.filter.resample.fs, bwe.decimate.factor = Q, fs, factor
    return args


def ops():
    iir, other = {}, {}
    for i, (order, sr, fc) in enumerate(CHEBY):
        args = tester_args("cheby1", fc=fc, order=order)
        b, a = ube.prepare_filter(args, sr)
        bn, an = normalise_fp32(b, a)
        ns = types.SimpleNamespace(a=torch.Tensor(a), b=torch.Tensor(b))
        x, w = inputs(100 + i)
        y, gx = op_and_grad(lambda v: Ref.apply_IIR_filter(ns, v), x, w)
        radius = float(np.abs(np.roots(an.double().numpy())).max())
        iir.update({f"cheby{i}_cfg": np.array([order, sr, fc, RIPPLE]), f"cheby{i}_seed": 100 + i, f"cheby{i}_b": b,
                    f"cheby{i}_a": a, f"cheby{i}_bn": bn, f"cheby{i}_an": an, f"cheby{i}_radius": radius,
                    f"cheby{i}_y": y, f"cheby{i}_gx": gx})
    fc, sr, Q = BIQUAD
    args = tester_args("biquad", fc=fc, Q=Q)
    c6 = ube.prepare_filter(args, sr)
    ns = types.SimpleNamespace(**{k: torch.Tensor(v.reshape(1)) for k, v in zip(("b0", "b1", "b2", "a0", "a1", "a2"), c6)})
    x, w = inputs(200, scale=2.0)
    y, gx = op_and_grad(lambda v: Ref.apply_biquad(ns, v), x, w)
    assert (y.abs() >= 1).any(), "the clamp must act in the biquad case"
    bn, an = normalise_fp32(torch.stack(list(c6[:3])), torch.stack(list(c6[3:])))
    other.update(biquad_cfg=np.array(BIQUAD), biquad_seed=200, biquad_scale=2.0, biquad_coef=torch.stack(list(c6)),
                 biquad_bn=bn, biquad_an=an, biquad_y=y, biquad_gx=gx)
    for i, fs in enumerate(RESAMPLE_FS):
        args = tester_args("resample", fs=fs)
        factor = ube.prepare_filter(args, 22050)
        ns = types.SimpleNamespace(factor=factor)
        x, w = inputs(300 + i)
        y, gx = op_and_grad(lambda v: Ref.resample(ns, v), x, w)
        other.update({f"resample{i}_fs": fs, f"resample{i}_factor": factor, f"resample{i}_seed": 300 + i,
                      f"resample{i}_y": y, f"resample{i}_gx": gx})
    for i, f in enumerate(DECIMATE):
        args = tester_args("decimate", factor=f)
        factor = ube.prepare_filter(args, 22050)
        ns = types.SimpleNamespace(factor=factor)
        x, w = inputs(400 + i, L=L_OPS + 3)
        y, gx = op_and_grad(lambda v: Ref.decimate(ns, v), x, w)
        other.update({f"decimate{i}_factor": factor, f"decimate{i}_fs_written": int(args.tester.bandwidth_extension.filter.resample.fs),
                      f"decimate{i}_seed": 400 + i, f"decimate{i}_y": y, f"decimate{i}_gx": gx})
    MG.save("degradation_ops_iir1k.npz", **{k: v for k, v in iir.items() if int(k[5]) < 3})
    MG.save("degradation_ops_iir3k.npz", **{k: v for k, v in iir.items() if int(k[5]) >= 3})
    MG.save("degradation_ops_other.npz", **other)


def sampler():
    out = {}
    L = 92092
    g = torch.Generator().manual_seed(1616)
    clean = 0.1 * torch.randn(1, L, generator=g)
    orig = torch.randn
    runs = [("cheby1", 0.05, False), ("cheby1_dc", 0.05, True), ("biquad", 0.05, False), ("resample", "None", False),
            ("decimate", "None", False)]
    for name, ss, dc in runs:
        ftype = name.split("_")[0]
        args = MG.small_args(T=3)
        args.tester.posterior_sampling.start_sigma = ss
        args.tester.posterior_sampling.data_consistency = dc
        net, sd = MG.build_ref_net(args)
        targs = tester_args(ftype, fc=3000, order=6, Q=0.707, fs=4000, factor=2)
        filt = ube.prepare_filter(targs, 22050)
        y = ube.apply_low_pass(clean, filt, ftype)
        with MG.quiet():
            s = Ref(MG.ResidualNetRef(net, 0.3, args.tester.diff_params.sigma_data), MG.edm_mod.EDM(args), args)
        seed = 1700 + len(out)
        gn = torch.Generator().manual_seed(seed)
        noises = [torch.randn(1, L, generator=gn) for _ in range(4)]
        it = iter(noises)
        torch.randn = lambda *a, **k: next(it)
        try:
            with MG.quiet(), contextlib.redirect_stderr(io.StringIO()):
                if ftype in ("resample", "decimate"):
                    x = s.predict_bwe(y.clone(), filt, ftype)
                    res = dict(x=x)
                else:
                    x, dden, dscore, t = s.predict_bwe(y.clone(), filt, ftype, rid=True)
                    res = dict(x=x, den_sub16=dden[:, :, ::16], score_sub16=dscore[:, :, ::16], t=t)
        finally:
            torch.randn = orig
        out[f"{name}_seed"] = seed
        if name != "cheby1_dc":                           # (same observations as 'cheby1')
            out[f"{name}_y"] = y
        res["x_sub4"] = res.pop("x")[:, ::4]
        out.update({f"{name}_{k}": v for k, v in res.items()})
    common = dict(clean_seed=1616, res_a=0.3)
    for fname, names in (("degradation_sampler_cheby1.npz", ("cheby1",)), ("degradation_sampler_biquad.npz", ("biquad",)),
                         ("degradation_sampler_rs.npz", ("resample", "decimate"))):
        MG.save(fname, **common, **{k: v for k, v in out.items() if k.split("_")[0] in names})


if __name__ == "__main__":
    which = sys.argv[1:] or ["ops", "sampler"]
    for w in which:
        globals()[w]()
