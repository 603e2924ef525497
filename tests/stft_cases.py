"""Cases and float64 references of the element-wise STFT / overlap-add / filter-fit tests (tests/test_stft_cases_cpu.py pins the
references on the CPU, tests/test_gpu_stft_edges.py runs the kernels of csrc/stft.hip against them).

Layout of the kernels (include/babe_hip.h): nfft zeros appended, hop nfft/2, periodic Hamming window w, frames = 1 + L // hop,
spectra [B][frames][nfft/2 + 1] complex, frames [B][frames][nfft], statistics [P][3][nbins] doubles (sum |X|^2, sum |X||Y|,
sum |Y|^2), filter parameters [P][2][K] float32 (row 0: fc in Hz, row 1: A in dB per octave).
"""
import numpy as np
import torch

from oracle import bwe_utils as U
from tests.fft_cases import BAR, Guarded, row_err  # noqa: F401  (the project's transform bar, the canaried buffers, the metric)

FS = 44100
B_TRANSFORM = 2

# (nfft, L, what the row reaches); every row runs with B = 2
TRANSFORM_CASES = [
    (256, 3 * 128 + 5, "64 radix-4 butterflies for 256 threads in every pass; last frame holds 5 samples"),
    (512, 3 * 256 + 5, "odd log2(n): the single radix-2 opening pass"),
    (1024, 3 * 512 + 5, "even log2(n), one butterfly per thread"),
    (2048, 3 * 1024 + 5, "odd log2(n), two butterflies per thread"),
    (4096, 3 * 2048 + 5, "the workload's size, four butterflies per thread"),
    (256, 100, "L < hop: one frame, no overlap anywhere"),
    (256, 128, "L = hop: two frames, the second all zero"),
    (256, 129, "one sample in the last frame"),
    (256, 383, "L = 3 hop - 1: the last frame is full to its first half, L % hop = hop - 1"),
    (256, 1000, "eight frames, L % hop = 104, several 256-thread blocks of the overlap-add"),
]
STRIDE_PAD = 7            # the strided case: x, y and the overlap-add output are rows of [B][L + 7] buffers


def transform_id(c):
    return f"nfft{c[0]}-L{c[1]}"


def n_frames(L, nfft):
    return 1 + L // (nfft // 2)


# ----------------------------------------------------------------------------- transforms and overlap-add (CPU, float64)
def window64(nfft):
    """torch.hamming_window(nfft) (periodic) in float64."""
    return 0.54 - 0.46 * torch.cos(2.0 * np.pi * torch.arange(nfft, dtype=torch.float64) / nfft)


def frames64(x, nfft):
    """[B, L] -> windowed frames [B, frames, nfft]."""
    x = x.double()
    xp = torch.cat((x, torch.zeros(x.shape[0], nfft, dtype=torch.float64)), dim=1)
    return xp.unfold(-1, nfft, nfft // 2)[:, : n_frames(x.shape[1], nfft)] * window64(nfft)


def stft64(x, nfft):
    """[B, L] -> complex128 [B, frames, nfft/2 + 1]."""
    return torch.fft.rfft(frames64(x, nfft), dim=-1)


def filtered_frames64(spec, H, nfft):
    """w * irfft(spec * H): spec complex [B, frames, bins] (ANY complex array: the imaginary parts at DC and Nyquist are
    ignored), H [bins] or [B, bins] (or the scalar 1) -> [B, frames, nfft]."""
    H = torch.as_tensor(H, dtype=torch.float64)
    Z = (spec.to(torch.complex128) * (H[:, None, :] if H.dim() == 2 else H)).clone()
    Z[..., 0] = Z[..., 0].real.to(torch.complex128)
    Z[..., -1] = Z[..., -1].real.to(torch.complex128)
    return torch.fft.irfft(Z, n=nfft, dim=-1) * window64(nfft)


def env_inv64(nfft, frames):
    """1 / (sum of the squared windows of all frames), length nfft + hop (frames - 1)."""
    hop = nfft // 2
    env = torch.zeros(nfft + hop * (frames - 1), dtype=torch.float64)
    for t in range(frames):
        env[t * hop: t * hop + nfft] += window64(nfft) ** 2
    return 1.0 / env


def ola64(frames, L, env_inv=None, y=None):
    """Overlap-add of [B, frames, nfft] at hop nfft/2, times env_inv if given, cropped to L; with y: (y - ola, sum of squares
    per clip)."""
    frames = frames.double()
    B, T, n = frames.shape
    hop = n // 2
    out = torch.zeros(B, n + hop * (T - 1), dtype=torch.float64)
    for t in range(T):
        out[:, t * hop: t * hop + n] += frames[:, t]
    if env_inv is not None:
        out = out * env_inv.double()[: out.shape[1]]
    out = out[:, :L]
    if y is None:
        return out
    r = y.double() - out
    return r, (r * r).sum(1)


def stats64(specX, specY, shared):
    """Complex [B, frames, bins] pair -> [B, 3, bins] (or [1, 3, bins] summed over the batch too) float64."""
    mx, my = specX.to(torch.complex128).abs(), specY.to(torch.complex128).abs()
    s = torch.stack([(mx * mx).sum(1), (mx * my).sum(1), (my * my).sum(1)], 1)
    return s.sum(0, keepdim=True) if shared else s


def as_complex(spec):
    """Planar-last float [..., 2] -> complex128 on the CPU."""
    spec = spec.double().cpu()
    return torch.complex(spec[..., 0], spec[..., 1])


def _rows_err(got, ref):
    """max over the rows of row_err.  Where the reference is exactly zero the result must be exactly zero: asserted here, and
    the rows that are zero throughout are left out of the relative errors.  NaN if any result is NaN."""
    assert bool((got[ref == 0] == 0).all()), "an element whose reference is exactly zero did not come back exactly zero"
    keep = ~(ref == 0).all(1)
    if not bool(keep.any()):
        return 0.0
    e = row_err(got[keep], ref[keep])
    return float("nan") if any(np.isnan(v) for v in e) else max(e)


def framed_err(got, ref):
    """max|got - ref| / max|ref| per clip AND per frame (or whatever the second axis is), the largest of them."""
    rows = got.shape[0] * got.shape[1]
    return _rows_err(got.reshape(rows, -1), ref.reshape(rows, -1))


def sample_err(got, ref):
    """max|got - ref| / max|ref| per clip, the largest of them."""
    return _rows_err(got.reshape(got.shape[0], -1), ref.reshape(ref.shape[0], -1))


def transform_inputs(nfft, L, B=B_TRANSFORM, seed=0):
    """x, y [B, L] float32, a RANDOM complex spectrum [B, frames, bins, 2] float32 (not the STFT of any real signal: its DC and
    Nyquist bins have imaginary parts), distinct per-clip filters H [B, bins] in (0.25, 1.25)."""
    g = torch.Generator().manual_seed(1000 * nfft + L + seed)
    T, nb = n_frames(L, nfft), nfft // 2 + 1
    x, y = 0.1 * torch.randn(B, L, generator=g), 0.1 * torch.randn(B, L, generator=g)
    spec = torch.randn(B, T, nb, 2, generator=g)
    H = 0.25 + torch.rand(B, nb, generator=g)
    return x, y, spec, H


# ----------------------------------------------------------------------------- one step of the fit (CPU, float64)
FIT_DEFAULTS = dict(mu=(100.0, 1.0), fcmin=20.0, fcmax=22050.0, Amin=-50.0, Amax=30.0, clamp_fc=True, clamp_A=True,
                    only_negative_A=True, weighting="sqrt")


def fit_objective64(stats, p, f64, weighting):
    """sqrt(sum_k w_k^2 (H_k^2 Sxx_k - 2 H_k Sxy_k + Syy_k)) with H = design_filter(p) in float64 (differentiable in p)."""
    H = U.design_filter(p[0], p[1], f64)
    w2 = U.freq_weight(f64.numel(), weighting).double() ** 2
    Sxx, Sxy, Syy = stats.double()
    return torch.sqrt((w2 * (H * H * Sxx - 2.0 * H * Sxy + Syy)).sum())


def project64(q, c):
    """The projection of oracle.bwe_utils.fit_params, in its order, with the switches filter_fit_kernel reads."""
    K = q.shape[1]
    if c["clamp_fc"]:
        q[0, 0] = q[0, 0].clamp(c["fcmin"], c["fcmax"])
        for k in range(1, K):
            q[0, k] = q[0, k].clamp(float(q[0, k - 1]) + 1.0, c["fcmax"])
    if c["clamp_A"]:
        q[1, 0] = q[1, 0].clamp(c["Amin"], -1.0 if c["only_negative_A"] else c["Amax"])
        for k in range(1, K):
            q[1, k] = q[1, k].clamp(c["Amin"], float(q[1, k - 1]) if c["only_negative_A"] else c["Amax"])
    return q


def fit_step64(stats, params, f32_bin_freqs, cfg):
    """One iteration of BlindSampler.fit_params from the statistics [3, nbins]: (loss, grad [2, K], new_params [2, K]), all
    float64.  The masks `f >= fc` are those of the float32 bin frequencies and the float32 parameters (both converted exactly)."""
    c = {**FIT_DEFAULTS, **cfg}
    assert f32_bin_freqs.dtype == torch.float32
    p = params.float().double().clone().requires_grad_(True)
    loss = fit_objective64(stats, p, f32_bin_freqs.double(), c["weighting"])
    g, = torch.autograd.grad(loss, p)
    q = (p - torch.tensor(c["mu"], dtype=torch.float64)[:, None] * g).detach()
    return float(loss.detach()), g.detach(), project64(q, c)


def ulp32(v):
    """Spacing of float32 at |v| (float64 tensor in, float64 tensor out)."""
    return torch.from_numpy(np.spacing(np.abs(v.numpy()).astype(np.float32)).astype(np.float64))


def step_bounds(grad, new_params, mu, bar):
    """What a one-step result may deviate from fit_step64's: a gradient wrong by `bar` relative to its row's maximum moves a
    parameter by mu * bar * max|g|; the step and the projection in float32 add at most 2 ulp of the parameter."""
    b = torch.stack([mu[0] * bar * grad[0].abs().max().expand_as(grad[0]), mu[1] * bar * grad[1].abs().max().expand_as(grad[1])])
    return b + 2.0 * ulp32(new_params)


def synth_stats(f32_bin_freqs, seed, true=(2500.0, -25.0), noise=0.1, frames=12, scale=1.0):
    """[3, nbins] float64 from random positive magnitudes X over `frames` frames and Y = X H_true (1 + noise); no STFT."""
    g = torch.Generator().manual_seed(seed)
    nb = f32_bin_freqs.numel()
    X = scale * (torch.rand(nb, frames, generator=g).double() + 0.05)
    Ht = U.design_filter(torch.tensor([true[0]]), torch.tensor([true[1]]), f32_bin_freqs).double()
    Y = (X * Ht[:, None] * (1.0 + noise * torch.randn(nb, frames, generator=g).double())).abs()
    return torch.stack([(X * X).sum(1), (X * Y).sum(1), (Y * Y).sum(1)])


def random_params(K, seed):
    """Sorted fc in (300, 15300) Hz, non-increasing A in (-35, -5) dB per octave, float32 [2, K]."""
    g = torch.Generator().manual_seed(seed)
    fc = torch.sort(300.0 + 15000.0 * torch.rand(K, generator=g)).values
    A = -torch.sort(5.0 + 30.0 * torch.rand(K, generator=g)).values
    return torch.stack([fc, A]).float()


def _fit(name, K, nfft, what, fs=FS, seed=None, params=None, true=(2500.0, -25.0), on_bin=False, **cfg):
    return dict(name=name, K=K, nfft=nfft, fs=fs, seed=seed, params=params, true=true, on_bin=on_bin, what=what, cfg=cfg)


# One descent step, both kernels.  params: explicit parameter sets [[fc...], [A...]] (one per launch row), else one random sorted
# set from the seed.  Everything not named is FIT_DEFAULTS (sqrt weighting, mu = (100, 1), every clamp on).
FIT_CASES = (
    [_fit(f"K{K}-nfft4096", K, 4096, f"filter_fit_fast_kernel<{K}> at the workload's 2049 bins", seed=100 * K) for K in range(1, 9)]
    + [_fit(f"K{K}-nfft{n}", K, n, f"{n // 2 + 1} bins: lanes tid + 256 m past the end, m >= {(n // 2 + 1 + 255) // 256}", seed=100 * K + n)
       for n in (1024, 256) for K in (1, 5, 8)]
    + [_fit(f"weighting-{w}", 3, 4096, f"weight_sq kind {w}", seed=31 + i, weighting=w) for i, w in enumerate(("None", "linear", "log"))]
    + [
        _fit("no-clamp_fc", 3, 4096, "clamp_fc = 0: fc stays outside [fcmin, fcmax] = [5000, 6000]", seed=41,
             clamp_fc=False, fcmax=6000.0, fcmin=5000.0),
        _fit("no-clamp_A", 3, 4096, "clamp_A = 0: A is neither bounded by Amin = -10 nor ordered", seed=42, clamp_A=False, Amin=-10.0),
        _fit("positive-A", 3, 4096, "only_negative_A = 0, Amax = 30: the observation is louder than the input above 2.5 kHz, the step "
             "drives A above zero (A[0] up to Amax)", params=[[[1500.0, 4000.0, 9000.0], [-0.4, -0.2, -0.3]]], seed=43, true=(2500.0, 6.0),
             only_negative_A=False, Amax=30.0, mu=(100.0, 4.0)),
        _fit("every-clamp", 4, 4096, "fc[0] -> fcmin, fc[1] -> fc[0] + 1, fc[3] -> fcmax, A[1] -> A[0], A[3] -> Amin",
             params=[[[1000.0, 1200.0, 5000.0, 9000.0], [-10.0, -5.0, -12.0, -30.0]]], seed=44, fcmin=3000.0, fcmax=8000.0, Amin=-20.0),
        _fit("P3", 3, 4096, "three statistics and parameter sets in one launch: the per-set offset ((long)p * 3 + i) * nbins",
             params=[[[800.0, 2100.0, 6100.0], [-6.0, -14.0, -22.0]], [[3100.0, 3900.0, 12000.0], [-9.0, -11.0, -30.0]],
                     [[450.0, 7000.0, 15000.0], [-3.0, -18.0, -40.0]]], seed=45),
        _fit("same-bin", 3, 4096, "breakpoints 1 Hz apart between bins 93 and 94: one kstar for all, two one-bin-less segments",
             params=[[[1003.0, 1004.0, 1005.0], [-5.0, -10.0, -20.0]]], seed=46),
        _fit("nyquist", 2, 4096, "fc[K-1] = 22050 = the last bin exactly: kstar = nbins - 1, a one-bin segment",
             params=[[[5000.0, 22050.0], [-10.0, -20.0]]], seed=47, on_bin=True),
        _fit("below-bin-1", 2, 4096, "fc[0] = 3 Hz < df: kstar = 1, every bin but DC in a segment, the step lands on fcmin",
             params=[[[3.0, 4000.0], [-3.0, -9.0]]], seed=48),
        _fit("on-bin", 3, 4096, "fs / nfft = 8 Hz exactly and fc ON bins 100, 300, 1000: the masks' >= side", fs=32768,
             params=[[[800.0, 2400.0, 8000.0], [-6.0, -12.0, -20.0]]], seed=49, fcmax=16384.0, on_bin=True),
    ])
FIT_BY_NAME = {c["name"]: c for c in FIT_CASES}
GRAD_KS = (1, 4, 8)       # 4b: the gradient read off an unclamped step with mu = (1, 1)
GRAD_SCALE = 1.0e5       # magnitudes of the 4b statistics: the gradient scales with them, and has to stand clear of the
                          # float32 spacing of fc (1e-3 Hz at 10 kHz) for a 5e-4 error in one of its terms to show


def fit_inputs(c, scale=1.0):
    """(stats [P, 3, nbins] float64, params [P, 2, K] float32, float32 bin frequencies, cfg dict) of one row of FIT_CASES."""
    f = U.bin_freqs(c["nfft"], c["fs"])
    params = torch.tensor(c["params"], dtype=torch.float32) if c["params"] is not None else random_params(c["K"], c["seed"])[None]
    stats = torch.stack([synth_stats(f, c["seed"] + 1000 * p, true=c["true"], scale=scale) for p in range(params.shape[0])])
    return stats, params.contiguous(), f, {**FIT_DEFAULTS, **c["cfg"]}


def grad_inputs(K):
    """4b: the K-at-2049-bins row with every clamp off and mu = (1, 1), statistics of magnitudes GRAD_SCALE times larger."""
    stats, params, f, cfg = fit_inputs(FIT_BY_NAME[f"K{K}-nfft4096"], scale=GRAD_SCALE)
    return stats, params, f, {**cfg, "mu": (1.0, 1.0), "clamp_fc": False, "clamp_A": False}


def exact_inputs(K=3, tol=5e-3, mu=(1000.0, 10.0)):
    """4c: statistics with Y = X H(p*) exactly, to be started at p* under the default mu and tolerances.  The residual the kernels
    see is then the rounding of their own float32 H, and the gradient of a 2-norm at such a residual is a direction of no
    particular smallness: J^T r / |r|, bounded by the column norms |J_j| of J = d(w sqrt(Sxx) H)/dp_j whatever r is.  The
    magnitudes are scaled so that mu_j |J_j| <= tol / 8 for every parameter: every step is then shorter than tol / 8, the
    second iteration meets the stopping rule, and two steps end within tol / 4 of p*."""
    f = U.bin_freqs(4096, FS)
    p = torch.tensor([[1800.0, 4200.0, 9100.0], [-8.0, -15.0, -24.0]])[:, :K].contiguous()
    s = synth_stats(f, 77)
    w = U.freq_weight(f.numel(), "sqrt").double()
    J = torch.autograd.functional.jacobian(lambda q: w * torch.sqrt(s[0]) * U.design_filter(q[0], q[1], f.double()), p.double())
    colnorm = J.reshape(f.numel(), 2, K).norm(dim=0)                                   # [2, K]
    scale = float((tol / 8.0 / (torch.tensor(mu, dtype=torch.float64)[:, None] * colnorm)).min())
    H = U.design_filter(p[0].double(), p[1].double(), f.double())
    Sxx = s[0] * scale ** 2
    return torch.stack([Sxx, H * Sxx, H * H * Sxx])[None], p[None].contiguous(), f, {**FIT_DEFAULTS, "mu": mu}


# 4d: design_filter rows [[fc...], [A...]], run at nfft 256 and 4096
DESIGN_CASES = {
    "K8-sorted": [[400.0, 700.0, 1300.0, 2500.0, 4100.0, 7300.0, 11000.0, 16000.0], [-2.0, -3.0, -4.0, -6.0, -8.0, -9.0, -10.0, -12.0]],
    "same-bin": [[1003.0, 1004.0, 1005.0], [-5.0, -10.0, -20.0]],
    "unsorted-older-value": [[5000.0, 2000.0, 9000.0], [-6.0, -10.0, -14.0]],      # anchor 1 sits below fc[0]: H there is still 1
    "unsorted-step-down": [[2000.0, 9000.0, 5000.0], [-6.0, -10.0, -14.0]],        # anchor 2 sits below fc[1]: written by segment 0
}


# ----------------------------------------------------------------------------- direct C-ABI calls (GPU)
def guarded_f64(n, src=None):
    """Guarded buffer of n doubles (its canaries and its NaN fill are NaN as doubles too)."""
    gd = Guarded(2 * n)
    if src is not None:
        gd.mid.view(torch.float64).copy_(src.reshape(-1))
    return gd


class Direct:
    """The kernels of csrc/stft.hip through the C-ABI with EVERY operand between canaries (tests.fft_cases.Guarded): inputs lie
    between NaNs, outputs are pre-filled with NaN, and after each call every canary must be intact.  Results come back on the
    CPU.  `stride`: x, y and the overlap-add output as rows of a [B][stride] buffer (the gaps keep their NaN)."""

    def __init__(self, nfft, L, fs=FS):
        from babe_amd.stft import STFTOps
        self.st = STFTOps(nfft, L, fs, "cuda")
        self.nfft, self.L, self.T, self.nb, self.nblk = nfft, L, self.st.frames, self.st.nbins, self.st.NBLK
        self.tw = Guarded(self.st.tw4096.numel(), src=self.st.tw4096)
        self.env = Guarded(self.st.env_inv.numel(), src=self.st.env_inv)

    def _call(self, name, bufs, *args):
        from babe_amd._lib import lib, stream
        rc = getattr(lib(), name)(*args, stream())
        torch.cuda.synchronize()
        assert rc == 0, (name, rc, lib().babe_last_error())
        for what, gd in list(bufs.items()) + [("twiddles", self.tw), ("envelope", self.env)]:
            assert gd.canaries_intact(), f"{name}: the call wrote outside its {what} buffer"

    def _rows(self, t, stride):
        """Guarded copy of t [B, L] as rows `stride` apart."""
        gd = Guarded(t.shape[0] * stride)
        gd.mid.view(t.shape[0], stride)[:, : t.shape[1]].copy_(t)
        return gd

    def stft(self, x, stride=None, pre=False):
        B, stride = x.shape[0], stride or self.L
        xin, out = self._rows(x, stride), Guarded(B * self.T * self.nb * 2, canary=-3.0)
        self._call("babe_stft_fwd", dict(x=xin, spec=out), xin.mid.data_ptr(), stride, self.L, self.env.mid.data_ptr() if pre else None,
                   out.mid.data_ptr(), B, self.nfft, self.T, self.tw.mid.data_ptr())
        return out.mid.cpu().reshape(B, self.T, self.nb, 2)

    def filter_frames(self, spec, H):
        B = spec.shape[0]
        sp, Hd, out = Guarded(spec.numel(), src=spec), Guarded(H.numel(), src=H), Guarded(B * self.T * self.nfft, canary=-3.0)
        self._call("babe_spec_filter_istft", dict(spec=sp, H=Hd, frames=out), sp.mid.data_ptr(), Hd.mid.data_ptr(),
                   0 if H.dim() == 1 else self.nb, out.mid.data_ptr(), B, self.nfft, self.T, self.tw.mid.data_ptr())
        return out.mid.cpu().reshape(B, self.T, self.nfft)

    def ola(self, fr, normalise, y=None, stride=None):
        B, stride = fr.shape[0], stride or self.L
        fin, out = Guarded(fr.numel(), src=fr), Guarded(B * stride, canary=-3.0)
        bufs = dict(frames=fin, out=out)
        yin = part = None
        if y is not None:
            yin, part = self._rows(y, stride), guarded_f64(B * self.nblk)
            bufs.update(y=yin, part=part)
        self._call("babe_ola", bufs, fin.mid.data_ptr(), self.env.mid.data_ptr() if normalise else None,
                   yin.mid.data_ptr() if y is not None else None, stride if y is not None else 0, out.mid.data_ptr(), stride,
                   part.mid.data_ptr() if y is not None else None, self.nblk, B, self.L, self.nfft, self.T)
        rows = out.mid.cpu().reshape(B, stride)
        assert bool(torch.isnan(rows[:, self.L:]).all()), "ola wrote between the rows of its strided output"
        res = rows[:, : self.L].contiguous()
        return (res, part.mid.view(torch.float64).cpu().reshape(B, self.nblk)) if y is not None else res

    def residual_seed(self, r, part, post):
        B = r.shape[0]
        rin, pin, out = Guarded(r.numel(), src=r), guarded_f64(part.numel(), src=part), Guarded(r.numel(), canary=-3.0)
        self._call("babe_residual_seed", dict(r=rin, part=pin, out=out), rin.mid.data_ptr(), self.L, pin.mid.data_ptr(), part.shape[1],
                   self.env.mid.data_ptr() if post else None, out.mid.data_ptr(), self.L, B, self.L)
        return out.mid.cpu().reshape(B, self.L)

    def mag_stats(self, X, Y, shared):
        B = X.shape[0]
        Bo = 1 if shared else B
        xin, yin, out = Guarded(X.numel(), src=X), Guarded(Y.numel(), src=Y), guarded_f64(Bo * 3 * self.nb)
        self._call("babe_stft_mag_stats", dict(specX=xin, specY=yin, stats=out), xin.mid.data_ptr(), yin.mid.data_ptr(),
                   out.mid.data_ptr(), B, self.nb, self.T, int(shared))
        return out.mid.view(torch.float64).cpu().reshape(Bo, 3, self.nb)


def run_fit(stats, params, c_nfft, c_fs, cfg, kernel, max_iter=1):
    """STFTOps.filter_fit on copies: (updated params [P, 2, K] float32 on the CPU, n_iter list)."""
    from babe_amd.stft import STFTOps, make_fit_cfg
    st = STFTOps(c_nfft, c_nfft, c_fs, "cuda")
    p = params.clone().cuda()
    nit = st.filter_fit(stats.cuda(), p, make_fit_cfg(**cfg, max_iter=max_iter, kernel=kernel))
    torch.cuda.synchronize()
    return p.cpu(), [int(v) for v in nit.cpu().tolist()]
