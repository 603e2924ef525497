"""Cases and float64 references of the CQT band and gather kernel tests (tests/test_cqt_cases_cpu.py pins both on the CPU,
tests/test_gpu_cqt_bands.py runs the kernels).

The kernels under test (csrc/cqt.hip; sequenced by babe_amd/cqt.py::CQT_nsgt or by csrc/cqt_plan.hip), in the terms of the header
of oracle/nsgt.py.  Band k of octave j has centre c, length M, window g[m] for m = -(M//2) .. M - M//2 - 1 and T = T_j coefficients:
  analysis  : planar half spectrum [B][2][KX] -> per octave [B][2][binsoct][T]:  T ifft_T(fold(X[(c + m) mod L] w[m])), X the full
              circle (conjugate mirror above L/2), fold puts offset m at m mod T;  w = g / T ("fwd") or gdual T 2 / L ("bwd_adjoint")
  synthesis : coefficients -> band spectra [B][nwin][2]: entry woff + mi = fft_T(c_k)[(mi - M//2) mod T] w[mi], woff = cumsum(M);
              w = gdual T ("bwd") or g / T ("fwd_adjoint")
  gather    : band spectra -> [B][2][KX]: scale mul[n] (P[n] + conj(P[L - n])), P the index-add of the entries at (c + m) mod L;
              the direct term alone at n = 0 and n = L/2; exactly 0 for L/2 < n < KX
  spec_scale: (s1 sc1 + s2 sc2) mul on 0 .. L/2, exactly 0 above
Geometry comes from oracle.nsgt.nsgt_design and kaiser_centered only: none of the tables babe_amd.cqt uploads (woff, rowptr, src,
rec, win_*) is read here, so that an error in those tables shows as well.
"""
import numpy as np
import torch

from oracle.nsgt import kaiser_centered, nsgt_design
from tests.fft_cases import BAR, GUARD, Guarded  # noqa: F401  (the GPU tests take them from here)

FS = 22050
WHOLE_BAR = 2e-5      # whole transforms against the oracle: the bar of tests/test_gpu_cqt.py, here per band and per clip

# id -> the design and what properties() must return for it (tests/test_cqt_cases_cpu.py compares value by value)
CASES = {
    # 7 bands wrap below bin 0, CSR gather with 18 sources on one bin, 16 bands fill their T, every band with T < 16
    "tiny": dict(L=64, N=(8, 8), numocts=6, binsoct=4, beta=1.0, T_oct=[4, 4, 4, 4, 8, 16],
                 wrap_low=7, mirror_high=1, max_sources=18, M_eq_4=18, M_eq_T=16, kdeg=5),
    # every one- and two-pass plan; CSR gather; 22 bands clamped to M = 4
    "short": dict(L=2048, N=(32, 64), numocts=8, binsoct=8, beta=1.0, T_oct=[4, 4, 8, 16, 32, 64, 128, 256],
                  wrap_low=0, mirror_high=1, max_sources=8, M_eq_4=22, M_eq_T=16, kdeg=5),
    # every three-pass plan; the longest band has 3668 samples; record gather
    "long": dict(L=20480, N=(128, 160), numocts=8, binsoct=4, beta=1.0, T_oct=[32, 64, 128, 256, 512, 1024, 2048, 4096],
                 wrap_low=0, mirror_high=1, max_sources=3, M_eq_4=0, M_eq_T=0, kdeg=5),
    # Kaiser polynomial of degree 7: the long Horner branch
    "deg7": dict(L=8192, N=(64, 128), numocts=4, binsoct=16, beta=2.0, T_oct=[64, 128, 256, 512],
                 wrap_low=0, mirror_high=1, max_sources=3, M_eq_4=0, M_eq_T=0, kdeg=7),
    # no analytic window: the table-reading kernels, in the class and in the plan (kdeg = 0)
    "table": dict(L=2048, N=(32, 64), numocts=5, binsoct=12, beta=6.0, T_oct=[8, 16, 32, 64, 128],
                  wrap_low=0, mirror_high=1, max_sources=3, M_eq_4=4, M_eq_T=0, kdeg=None),
    # record gather at a size where B = 9 is cheap
    "rec9": dict(L=2048, N=(32, 64), numocts=6, binsoct=8, beta=1.0, T_oct=[8, 16, 32, 64, 128, 256],
                 wrap_low=0, mirror_high=1, max_sources=3, M_eq_4=6, M_eq_T=0, kdeg=5),
}
PROPERTY_KEYS = ("T_oct", "wrap_low", "mirror_high", "max_sources", "M_eq_4", "M_eq_T", "kdeg")
ANALYSIS_KINDS = ("fwd", "bwd_adjoint")
SYNTHESIS_KINDS = ("bwd", "fwd_adjoint")


def ctor(case):
    """(args, kwargs) of either CQT_nsgt class for the case."""
    c = CASES[case]
    return (c["numocts"], c["binsoct"], "oct", ("kaiser", c["beta"]), FS, c["L"]), {}


def properties(case):
    """What the design reaches, from babe_amd.cqt.design_bands (the tables the kernels run on)."""
    from babe_amd.cqt import design_bands, kaiser_poly
    c = CASES[case]
    d = design_bands(FS, c["L"], c["numocts"], c["binsoct"], c["beta"])
    M, ctr, T, L = d["M"], d["c"], d["T"], c["L"]
    kp = kaiser_poly(c["beta"])
    return dict(T_oct=[int(T[j * c["binsoct"]]) for j in range(c["numocts"])],
                wrap_low=int((ctr - M // 2 < 0).sum()),
                mirror_high=int((ctr + M - M // 2 - 1 > L // 2).sum()),
                max_sources=int(np.diff(d["rowptr"]).max()),
                M_eq_4=int((M == 4).sum()), M_eq_T=int((M == T).sum()),
                kdeg=None if kp is None else int(kp[0]))


# ----------------------------------------------------------------------------- geometry and windows (float64, oracle only)
class Geometry:
    """Band geometry and the four window kinds of a case, from oracle.nsgt.nsgt_design and kaiser_centered."""

    def __init__(self, case):
        c = CASES[case]
        self.case, self.L, self.binsoct, self.numocts, self.beta = case, c["L"], c["binsoct"], c["numocts"], c["beta"]
        d = nsgt_design(FS, c["L"], c["numocts"], c["binsoct"], c["beta"])
        L = self.L
        self.nb = int(d["nb"])
        self.M, self.c, self.T = (np.asarray(d[k], dtype=np.int64) for k in ("M", "c", "T"))
        self.T_oct = [int(t) for t in d["T_oct"]]
        self.woff = np.concatenate(([0], np.cumsum(self.M)[:-1]))
        self.nwin = int(self.M.sum())
        N1 = c["N"][0]
        self.KX = ((L // 2) // N1 + 1) * N1
        self.m = [np.arange(-(int(Mk) // 2), int(Mk) - int(Mk) // 2) for Mk in self.M]
        self.idx = [(int(ck) + mk) % L for ck, mk in zip(self.c, self.m)]
        self.g = [kaiser_centered(int(Mk), self.beta) for Mk in self.M]
        # dual-frame diagonal over the full circle: every band and its mirror image, the DC and the Nyquist band
        diag = np.zeros(L)
        for k in range(self.nb):
            np.add.at(diag, self.idx[k], self.T[k] * self.g[k] ** 2)
            np.add.at(diag, (-self.idx[k]) % L, self.T[k] * self.g[k] ** 2)
        lp = np.zeros(L)
        for Mx, centre in ((int(d["M_dc"]), 0), (int(d["M_ny"]), L // 2)):
            gx = kaiser_centered(Mx, self.beta, symmetric=True)
            np.add.at(lp, (centre + np.arange(-(Mx // 2), Mx // 2 + 1)) % L, Mx * gx * gx)
        self.diag = diag + lp
        self.hpf = (1.0 - lp / self.diag)[: L // 2 + 1]
        self.gdual = [self.g[k] / self.diag[self.idx[k]] for k in range(self.nb)]
        cw = np.full(L // 2 + 1, 2.0 / L)
        cw[0] = cw[-1] = 1.0 / L
        self.irfft_w = cw                                  # irfft(X) = rfft_T(irfft_w X)

    def window(self, k, kind):
        T = float(self.T[k])
        if kind in ("fwd", "fwd_adjoint"):
            return self.g[k] / T
        if kind == "bwd":
            return self.gdual[k] * T
        if kind == "bwd_adjoint":
            return self.gdual[k] * T * (2.0 / self.L)
        raise KeyError(kind)

    def bands_of(self, j):
        return range(j * self.binsoct, (j + 1) * self.binsoct)


_GEO = {}


def geometry(case):
    if case not in _GEO:
        _GEO[case] = Geometry(case)
    return _GEO[case]


# ----------------------------------------------------------------------------- inputs
def seed_of(case, salt=0):
    return 1000 * (list(CASES).index(case) + 1) + salt


def rand_spec(case, B, seed, nan_above=True):
    """Planar half spectrum [B][2][KX] (float32), the bins L/2 < n < KX NaN (a kernel that reads them poisons its result) or 0."""
    geo = geometry(case)
    g = torch.Generator().manual_seed(seed)
    s = torch.full((B, 2, geo.KX), float("nan") if nan_above else 0.0)
    s[:, :, : geo.L // 2 + 1] = torch.randn(B, 2, geo.L // 2 + 1, generator=g)
    return s


def rand_coefs(case, B, seed):
    geo = geometry(case)
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(B, 2, geo.binsoct, T, generator=g) for T in geo.T_oct]


def rand_bs(case, B, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, geometry(case).nwin, 2, generator=g)


def rand_mul(case, seed):
    g = torch.Generator().manual_seed(seed)
    return 0.5 + torch.rand(geometry(case).L // 2 + 1, generator=g)


# ----------------------------------------------------------------------------- float64 references of the stages
def full_circle(spec, L):
    """planar [B][2][KX] -> complex128 [B][L]: spec[n] up to L/2, conj(spec[L - n]) above.  Bins above L/2 of `spec` are not read."""
    s = spec.double()
    half = torch.complex(s[:, 0, : L // 2 + 1], s[:, 1, : L // 2 + 1])
    return torch.cat([half, torch.conj(torch.flip(half[:, 1: L // 2], dims=(-1,)))], -1)


def ref_analysis(case, spec, kind):
    """Per octave [B][2][binsoct][T] float64."""
    geo = geometry(case)
    X = full_circle(spec, geo.L)
    B = X.shape[0]
    out = []
    for j, T in enumerate(geo.T_oct):
        buf = torch.zeros(B, geo.binsoct, T, dtype=torch.complex128)
        for i, k in enumerate(geo.bands_of(j)):
            w = torch.from_numpy(geo.window(k, kind))
            buf[:, i, torch.from_numpy(geo.m[k] % T)] = X[:, torch.from_numpy(geo.idx[k])] * w
        co = T * torch.fft.ifft(buf, dim=-1)
        out.append(torch.stack([co.real, co.imag], 1))
    return out


def ref_synthesis(case, coefs, kind):
    """Band spectra [B][nwin][2] float64."""
    geo = geometry(case)
    B = coefs[0].shape[0]
    bs = torch.zeros(B, geo.nwin, dtype=torch.complex128)
    for j, T in enumerate(geo.T_oct):
        cj = coefs[j].double()
        F = torch.fft.fft(torch.complex(cj[:, 0], cj[:, 1]), dim=-1)                # [B][binsoct][T]
        for i, k in enumerate(geo.bands_of(j)):
            Mk = int(geo.M[k])
            pos = torch.from_numpy((np.arange(Mk) - Mk // 2) % T)
            bs[:, geo.woff[k]: geo.woff[k] + Mk] = F[:, i, pos] * torch.from_numpy(geo.window(k, kind))
    return torch.stack([bs.real, bs.imag], -1)


def ref_gather(case, bs, scale, mul=None):
    """[B][2][KX] float64, zero above L/2.  (The GPU tests pass the float32 value of `scale` that the kernel receives.)"""
    geo = geometry(case)
    L, B = geo.L, bs.shape[0]
    v = bs.double()
    v = torch.complex(v[..., 0], v[..., 1])
    P = torch.zeros(B, L, dtype=torch.complex128)
    P.index_add_(1, torch.from_numpy(np.concatenate(geo.idx)), v)
    S = P[:, : L // 2 + 1].clone()
    S[:, 1: L // 2] += torch.conj(torch.flip(P[:, L // 2 + 1:], dims=(-1,)))      # P[L - n], n = 1 .. L/2 - 1
    S = S * float(scale)
    if mul is not None:
        S = S * mul.double()
    out = torch.zeros(B, 2, geo.KX, dtype=torch.float64)
    out[:, 0, : L // 2 + 1], out[:, 1, : L // 2 + 1] = S.real, S.imag
    return out


def ref_spec_scale(case, s1, mul=None, sc1=1.0, s2=None, sc2=0.0):
    geo = geometry(case)
    n = geo.L // 2 + 1
    acc = s1.double()[:, :, :n] * float(sc1)
    if s2 is not None:
        acc = acc + s2.double()[:, :, :n] * float(sc2)
    if mul is not None:
        acc = acc * mul.double()
    out = torch.zeros(s1.shape[0], 2, geo.KX, dtype=torch.float64)
    out[:, :, :n] = acc
    return out


def spec_to_signal(case, spec):
    """rfft_T in float64: x[n] = Re sum_k (S[0][k] + i S[1][k]) e^{+2 pi i k n / L} over the bins 0 .. L/2."""
    geo = geometry(case)
    Z = torch.zeros(spec.shape[0], geo.L, dtype=torch.complex128)
    Z[:, : geo.L // 2 + 1] = torch.complex(spec[:, 0, : geo.L // 2 + 1].double(), spec[:, 1, : geo.L // 2 + 1].double())
    return geo.L * torch.fft.ifft(Z, dim=-1).real


def signal_to_spec(case, x):
    """rfft in float64 as a planar half spectrum [B][2][KX] (zero above L/2)."""
    geo = geometry(case)
    X = torch.fft.fft(x.double(), dim=-1)[:, : geo.L // 2 + 1]
    out = torch.zeros(x.shape[0], 2, geo.KX, dtype=torch.float64)
    out[:, 0, : geo.L // 2 + 1], out[:, 1, : geo.L // 2 + 1] = X.real, X.imag
    return out


def f32(v):
    """The float32 a C `float` argument receives, as a Python float."""
    return float(np.float32(v))


def max_sources(case):
    """Largest number of band entries (direct and mirrored) that land on one bin of 0 .. L/2."""
    geo = geometry(case)
    idx = np.concatenate(geo.idx)
    return int(np.bincount(np.where(idx <= geo.L // 2, idx, geo.L - idx), minlength=geo.L // 2 + 1).max())


# ----------------------------------------------------------------------------- the oracle (whole transforms, float64)
_ORC = {}


def oracle(case):
    from oracle.nsgt import CQT_nsgt as OracleCQT
    if case not in _ORC:
        a, kw = ctor(case)
        _ORC[case] = OracleCQT(*a, dtype=torch.float64, **kw)
    return _ORC[case]


def to_complex(co):
    """planar per-octave list -> the oracle's complex list [B][1][binsoct][T]."""
    return [torch.complex(c[:, 0].double().cpu(), c[:, 1].double().cpu()).unsqueeze(1) for c in co]


def to_planar(cl):
    return [torch.stack([c.squeeze(1).real, c.squeeze(1).imag], 1) for c in cl]


def oracle_fwd(case, x):
    return to_planar(oracle(case).fwd(x.double().unsqueeze(1)))


def oracle_bwd(case, co):
    return oracle(case).bwd(to_complex(co)).squeeze(1)


def oracle_fwd_adjoint(case, gco):
    """Gradient of <fwd(x), gco> (real inner product over both planes) w.r.t. x, by float64 autograd through the oracle."""
    L = CASES[case]["L"]
    x = torch.zeros(gco[0].shape[0], L, dtype=torch.float64, requires_grad=True)
    co = oracle(case).fwd(x.unsqueeze(1))
    s = sum((c.squeeze(1).real * g[:, 0].double()).sum() + (c.squeeze(1).imag * g[:, 1].double()).sum() for c, g in zip(co, gco))
    return torch.autograd.grad(s, x)[0]


def oracle_bwd_adjoint(case, gx):
    """Gradient of <bwd(c), gx> w.r.t. the planar coefficients."""
    geo = geometry(case)
    B = gx.shape[0]
    pl = [torch.zeros(B, 2, geo.binsoct, T, dtype=torch.float64, requires_grad=True) for T in geo.T_oct]
    y = oracle(case).bwd([torch.complex(p[:, 0], p[:, 1]).unsqueeze(1) for p in pl]).squeeze(1)
    return list(torch.autograd.grad((y * gx.double()).sum(), pl))


# ----------------------------------------------------------------------------- error measures
def _np(t):
    return t.detach().double().cpu().numpy()


def coef_band_err(got, ref):
    """[B][nb]: max|got - ref| / max|ref| over the T complex coefficients of every band of every clip.  `got`, `ref`: per-octave
    planar lists.  NaN (an element the kernel did not write, or one computed from a canary) stays NaN and fails every `<`."""
    out = []
    for g, r in zip(got, ref):
        g, r = _np(g), _np(r)
        d = np.hypot(g[:, 0] - r[:, 0], g[:, 1] - r[:, 1])                        # [B][binsoct][T]
        out.append(d.max(-1) / np.hypot(r[:, 0], r[:, 1]).max(-1))
    return np.concatenate(out, 1)


def bs_band_err(case, got, ref):
    """[B][nb]: the same over the M entries woff .. woff + M of every band's spectrum.  got, ref: [B][nwin][2]."""
    geo = geometry(case)
    g, r = _np(got), _np(ref)
    d, a = np.hypot(g[..., 0] - r[..., 0], g[..., 1] - r[..., 1]), np.hypot(r[..., 0], r[..., 1])
    return np.maximum.reduceat(d, geo.woff, axis=1) / np.maximum.reduceat(a, geo.woff, axis=1)


def clip_err(got, ref, planar_axis=None):
    """[B]: max|got - ref| / max|ref| per clip; planar_axis: the axis holding (re, im), compared as complex magnitudes."""
    g, r = _np(got), _np(ref)
    if planar_axis is not None:
        g, r = np.moveaxis(g, planar_axis, 0), np.moveaxis(r, planar_axis, 0)
        d, a = np.hypot(g[0] - r[0], g[1] - r[1]), np.hypot(r[0], r[1])
    else:
        d, a = np.abs(g - r), np.abs(r)
    B = d.shape[0]
    return d.reshape(B, -1).max(1) / a.reshape(B, -1).max(1)


def worst(err):
    """Largest entry, NaN if any is NaN."""
    return float(np.max(err))


# ----------------------------------------------------------------------------- guarded device buffers (GPU)
class GuardedCoefs:
    """The per-octave coefficient tensors [B][2][binsoct][T], each inside its own guarded buffer: as an output NaN-filled
    between canaries of -3, as an input (`src`) between NaNs."""

    def __init__(self, case, B, src=None):
        geo = geometry(case)
        self.bufs = [Guarded(B * 2 * geo.binsoct * T, canary=-3.0 if src is None else float("nan"), src=None if src is None else src[j])
                     for j, T in enumerate(geo.T_oct)]
        self.views = [gd.mid.view(B, 2, geo.binsoct, T) for gd, T in zip(self.bufs, geo.T_oct)]

    def canaries_intact(self):
        return all(gd.canaries_intact() for gd in self.bufs)
