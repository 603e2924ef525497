"""Cases, float64 references and error bounds of the per-element tests of the UNet layer path's streaming kernels: GroupNorm / FiLM /
GELU forward and input-VJP (csrc/norm.hip), the x1/2 and x2 resamplers and their adjoints (csrc/resample.hip) and the copy / add /
fill / linear kernels of csrc/misc.hip.  tests/test_layer_cases_cpu.py pins the references, the tables and the bounds without a
GPU; tests/test_gpu_layer_edges.py runs the kernels.  Importing this module needs no GPU: the helpers that call the library import
it inside the function, and hand it only `Guarded` buffers (tests/fft_cases.py).

eps: the entry points take it as a float, so the operation under test has eps = float32(1e-7); the references use that value.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import unet as UN
from tests.fft_cases import Guarded

U32 = 2.0 ** -24                                  # unit roundoff of float32
EPS = float(np.float32(1e-7))
NAN = float("nan")
GELU_BAR = 1e-6                                   # the project's bar on gelu_f (tests/test_gpu_ops.py), held for gelu_grad_f too
GELU_GRAD_MAX = 1.13                              # max |gelu'| (1.1289 at u = 1.41)


# ============================================================================= A. GroupNorm statistics and scale
# (B, C, G, F, T, n, S, what the row reaches)
GN_CASES = [
    (1, 8, 8, 1, 4, 4, 1, "smallest legal group; cg = 1; one float4; only the unrolled loop's tail"),
    (2, 16, 8, 5, 8, 80, 1, "B = 2; film as a column slice of a wider tensor (film_bs != C)"),
    (1, 24, 8, 683, 16, 32784, 2, "chunk 16392: the split boundary falls inside the middle channel of each group"),
    (1, 8, 8, 12289, 4, 49156, 3, "chunk 16388: the last split is short (16380); cg = 1"),
    (1, 1, 1, 640, 1024, 655360, 40, "second round of the 32-lane sum partly filled (G = 1)"),
    (1, 1, 1, 1024, 1024, 1 << 20, 64, "the clamp; two full rounds"),
]
REGIMES = ("unit", "integers", "offset", "tiny", "constant")
FORMS3 = ("two", "one", "folded")                 # gn_partial + gn_finalize; gn_stats; gn_partial + scale_gelu_fin
PART_SHAPE = (1, 8, 8, 5, 8)                      # n = 40: the direct babe_gn_partial + babe_gn_finalize calls
PART_SPLITS = (1, 2, 3, 7, 33, 64)
FILM_PAD = (2, 1)                                 # columns of the wide film tensor before / after the C that are read


def gn_id(c):
    return "x".join(str(v) for v in c[:5])


def gn_splits(n):
    """babe_gn_splits restated."""
    return min(max(n // 16384, 1), 64)


def gn_chunk(n, S):
    """Elements per split: the kernels' rule, a multiple of 4."""
    return ((n // 4 + S - 1) // S) * 4


def split_ranges(n, S):
    """[beg, end) of every split of a group of n elements; beg >= end: an empty split."""
    ch = gn_chunk(n, S)
    return [(s * ch, min(s * ch + ch, n)) for s in range(S)]


def _seed(*key):
    return int(sum((i + 1) * 7919 * int(v) for i, v in enumerate(key)) % (2 ** 31 - 1))


def gn_data(regime, B, C, G, Fq, T):
    """x [B, C, Fq, T] float32 of one data regime, seeded by regime and shape."""
    g = torch.Generator().manual_seed(_seed(REGIMES.index(regime), B, C, Fq, T))
    shape = (B, C, Fq, T)
    if regime == "unit":
        return 1.7 * torch.randn(shape, generator=g) + 0.4
    if regime == "integers":
        return torch.randint(-3, 4, shape, generator=g).float()
    if regime == "offset":
        return 128.0 + torch.randint(-1, 2, shape, generator=g).float()
    if regime == "tiny":
        return 3e-7 * torch.randn(shape, generator=g)
    assert regime == "constant"                   # group 0: all 0.5; group 1 (if there is one): all 0; the rest as `unit`
    x = (1.7 * torch.randn(shape, generator=g) + 0.4).reshape(B * G, -1)
    x[0] = 0.5
    if B * G > 1:
        x[1] = 0.0
    return x.reshape(shape).contiguous()


def gn_params(B, C, pow2=False):
    """gamma [C] and a WIDE film tensor [B, 2 + C + 1] whose columns 2 .. 2 + C are the film that is read (film_bs = C + 3); the
    other columns are NaN.  pow2: gamma a power of two and film + 1 = 1 (exact products)."""
    g = torch.Generator().manual_seed(_seed(11, B, C))
    wide = torch.full((B, FILM_PAD[0] + C + FILM_PAD[1]), NAN)
    if pow2:
        gamma = 2.0 ** torch.randint(-2, 3, (C,), generator=g).float()
        wide[:, FILM_PAD[0]:FILM_PAD[0] + C] = 0.0
    else:
        gamma = 1 + 0.2 * torch.randn(C, generator=g)
        wide[:, FILM_PAD[0]:FILM_PAD[0] + C] = 0.3 * torch.randn(B, C, generator=g)
    return gamma, wide


def film_of(wide, C):
    return wide[:, FILM_PAD[0]:FILM_PAD[0] + C]


def gelu64(u):
    return F.gelu(u.double())


def gelu_grad64(u):
    u = u.double()
    return 0.5 * (1 + torch.erf(u / math.sqrt(2.0))) + u * torch.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi)


def gn_ref64(x, gamma, film, G):
    """float64 statistics, scale and output of the forward: mean, std [B, G]; scale [B, C]; u = x * scale; a = gelu(u)."""
    B, C, Fq, T = x.shape
    xg = x.double().reshape(B, G, -1)
    mean, std = xg.mean(-1), xg.std(-1)
    r = 1.0 / (std + EPS)
    scale = gamma.double()[None, :] * (film.double() + 1) * r.repeat_interleave(C // G, dim=1)
    u = x.double() * scale[:, :, None, None]
    return dict(mean=mean, std=std, r=r, scale=scale, u=u, a=gelu64(u))


def ulps32(got, ref64):
    """|got - ref64| in units of the float32 spacing at |ref64|."""
    ref = ref64.double()
    sp = np.spacing(np.abs(ref.numpy()).astype(np.float32)).astype(np.float64)
    return (got.double() - ref).abs() / torch.from_numpy(sp).reshape(ref.shape)


def fwd_bound(u64):
    """B: |a - gelu64(u64)| <= 1e-6 + 8 * 2^-24 * |u64|: the bar on gelu_f plus 7 ulp on its argument (4 on the scale, the product,
    and the reference's own rounding) times max |gelu'| = 1.13."""
    return GELU_BAR + 8 * U32 * u64.abs()


# ---- the kernels' arithmetic restated in float32 on the CPU (what a correct kernel may differ from float64 by)
def _f(v):
    return torch.tensor(v, dtype=torch.float32)


def phi_pdf32(u):
    """csrc/gelu.h phi_pdf in torch float32 (exp and a true division in place of the hardware's fast forms)."""
    ax = u.abs() * _f(0.70710678118654752440)
    E = torch.exp(_f(-0.5) * u * u)
    t = _f(1.0) / (_f(0.3275911) * ax + _f(1.0))
    P = _f(1.061405429) * t + _f(-1.453152027)
    for c in (1.421413741, -0.284496736, 0.254829592):
        P = P * t + _f(c)
    P = _f(0.5) * P * t * E
    return torch.where(u >= 0, _f(1.0) - P, P), E


def gelu32(u):
    return u * phi_pdf32(u)[0]


def gelu_grad32(u):
    Phi, E = phi_pdf32(u)
    return u * _f(0.39894228040143267794) * E + Phi


def gn_restate32(x, gamma, film, G):
    """gn_stat and the scale as the kernels form them: sums in double, mean / std rounded to float, r, scale and a in float32."""
    B, C, Fq, T = x.shape
    n = (C // G) * Fq * T
    xg = x.double().reshape(B, G, -1)
    s0, s1 = xg.sum(-1), (xg * xg).sum(-1)
    mean = s0 / n
    var = ((s1 - n * mean * mean) / (n - 1)).clamp_min(0.0)
    sd = var.sqrt().float()
    r = _f(1.0) / (sd + _f(EPS))
    scale = gamma[None, :] * (film + _f(1.0)) * r.repeat_interleave(C // G, dim=1)
    stats = torch.stack([mean.float(), sd, r], -1)
    return dict(part=torch.stack([s0, s1], -1), stats=stats, scale=scale, a=gelu32(x * scale[:, :, None, None]))


# ---- direct C-ABI calls (GPU)
class Canaried:
    """The Guarded buffers of one direct call; check() waits for the GPU and asserts that every canary came back."""

    def __init__(self):
        self.items = []

    def f32(self, name, src=None, n=None, fill=NAN):
        gd = Guarded(src.numel() if src is not None else n, fill=fill, src=src.float() if src is not None else None)
        self.items.append((name, gd))
        return gd

    def f64(self, name, n):
        """n doubles, NaN as doubles"""
        gd = Guarded(2 * n)
        gd.mid.view(torch.float64).fill_(NAN)
        self.items.append((name, gd))
        return gd

    def check(self, what):
        torch.cuda.synchronize()
        for name, gd in self.items:
            assert gd.canaries_intact(), f"{what}: the call wrote outside its {name} buffer"


def _p(gd, off=0):
    """device address of element `off` (in floats) of a Guarded buffer's payload"""
    return gd.mid.data_ptr() + 4 * off


def gn_forward(form, x, gamma, wide, G, S=None):
    """The forward in one of FORMS3, every operand canaried, film a column slice of `wide`.  dict of CPU tensors: part [B*G, S, 2]
    (float64), stats [B, G, 3], scale [B, C], a like x."""
    from babe_amd._lib import check, lib, stream
    B, C, Fq, T = x.shape
    hw, n = Fq * T, (C // G) * Fq * T
    S = S or gn_splits(n)
    k = Canaried()
    xg, gm, fw = k.f32("x", x), k.f32("gamma", gamma), k.f32("film", wide)
    part, stats, scale, a = k.f64("part", B * G * S * 2), k.f32("stats", n=B * G * 3), k.f32("scale", n=B * C), k.f32("a", n=x.numel())
    film, fbs = _p(fw, FILM_PAD[0]), wide.shape[1]
    L, st = lib(), stream()
    if form == "one":
        ticket = k.f32("ticket", n=B * G, fill=0.0)
        check(L.babe_gn_stats(_p(xg), _p(part), _p(ticket), _p(gm), film, fbs, _p(stats), _p(scale), B, C, G, n, S, EPS, st), "gn_stats")
    else:
        check(L.babe_gn_partial(_p(xg), _p(part), B, G, n, S, st), "gn_partial")
    if form == "two":
        check(L.babe_gn_finalize(_p(part), _p(gm), film, fbs, _p(stats), _p(scale), B, C, G, n, S, EPS, st), "gn_finalize")
    if form == "folded":
        check(L.babe_scale_gelu_fin(_p(xg), _p(part), _p(gm), film, fbs, _p(stats), _p(scale), _p(a), B, C, G, hw, S, EPS, st),
              "scale_gelu_fin")
    else:
        check(L.babe_scale_gelu(_p(xg), _p(scale), _p(a), B, C, hw, st), "scale_gelu")
    k.check(f"gn_forward {form} {tuple(x.shape)}")
    if form == "one":
        assert int(ticket.mid.view(torch.int32).abs().sum()) == 0, "gn_stats left a ticket non-zero"
    return dict(part=part.mid.view(torch.float64).cpu().reshape(B * G, S, 2), stats=stats.mid.cpu().reshape(B, G, 3),
                scale=scale.mid.cpu().reshape(B, C), a=a.mid.cpu().reshape(x.shape))


def gn_partial_finalize(x, gamma, wide, G, S):
    """babe_gn_partial + babe_gn_finalize with a caller-chosen S: (part [B*G, S, 2], stats, scale)."""
    from babe_amd._lib import check, lib, stream
    B, C, Fq, T = x.shape
    n = (C // G) * Fq * T
    k = Canaried()
    xg, gm, fw = k.f32("x", x), k.f32("gamma", gamma), k.f32("film", wide)
    part, stats, scale = k.f64("part", B * G * S * 2), k.f32("stats", n=B * G * 3), k.f32("scale", n=B * C)
    L, st = lib(), stream()
    check(L.babe_gn_partial(_p(xg), _p(part), B, G, n, S, st), "gn_partial")
    check(L.babe_gn_finalize(_p(part), _p(gm), _p(fw, FILM_PAD[0]), wide.shape[1], _p(stats), _p(scale), B, C, G, n, S, EPS, st),
          "gn_finalize")
    k.check(f"gn_partial_finalize S={S}")
    return part.mid.view(torch.float64).cpu().reshape(B * G, S, 2), stats.mid.cpu().reshape(B, G, 3), scale.mid.cpu().reshape(B, C)


# ============================================================================= B. scale_gelu_units
UNITS_CASES = [(2, 8, 1, 4, "Q = 1: one thread writes both zero borders"), (2, 8, 1, 8, "Q = 2: first and last thread differ")]
BF16_NAN = 0x7FC0


def units_expected(a):
    """The bf16 units of a [B, C, F, T] (float32) as int16 [B, C/8, F, 4, T/4 + 1, 8]: plane p entry j = time 4j + p - 1, zero for
    t = -1 and t >= T."""
    B, C, Fq, T = a.shape
    PI = T // 4 + 1
    bits = a.to(torch.bfloat16).view(torch.int16).reshape(B, C // 8, 8, Fq, T)
    out = torch.zeros(B, C // 8, Fq, 4, PI, 8, dtype=torch.int16)
    for p in range(4):
        for j in range(PI):
            t = 4 * j + p - 1
            if 0 <= t < T:
                out[:, :, :, p, j, :] = bits[:, :, :, :, t].permute(0, 1, 3, 2)
    return out


def units_call(x, scale, slack=24):
    """(a of babe_scale_gelu, the whole int16 buffer of babe_scale_gelu_units pre-filled with bf16 NaN and `slack` int16 longer
    than B * babe_units_size * 8, that size)."""
    from babe_amd._lib import check, lib, stream
    B, C, Fq, T = x.shape
    L, st = lib(), stream()
    nu = int(L.babe_units_size(C, Fq, T)) * 8 * B
    assert nu % 2 == 0 and slack % 2 == 0
    k = Canaried()
    xg, sg, a, au = k.f32("x", x), k.f32("scale", scale), k.f32("a", n=x.numel()), k.f32("units", n=(nu + slack) // 2)
    au.mid.view(torch.int16).fill_(BF16_NAN)
    check(L.babe_scale_gelu(_p(xg), _p(sg), _p(a), B, C, Fq * T, st), "scale_gelu")
    check(L.babe_scale_gelu_units(_p(xg), _p(sg), _p(au), B, C, Fq, T, st), "scale_gelu_units")
    k.check(f"units {tuple(x.shape)}")
    return a.mid.cpu().reshape(x.shape), au.mid.view(torch.int16).cpu(), nu


# ============================================================================= C. GroupNorm input-VJP
VJP_CASES = [(c, r) for c in GN_CASES[:4] for r in ("unit", "tiny")] + [(GN_CASES[1], "offset")]
VJP_VARIANTS = (("none", 0.0), ("alias", 0.5), ("separate", 0.5), ("separate", 0.0))      # (gy, rbeta)
# The constant c of the per-element bound: twice the largest value the kernel-order float32 restatement (vjp_restate32) needs over
# VJP_CASES x VJP_VARIANTS x {GELU, no GELU}, c = max (|gx32 - gx64| - 1e-6 tg) / (2^-24 t32), measured on the CPU by
# tests/test_layer_cases_cpu.py::test_vjp_restatement_stays_inside_the_bound (largest over the four gy variants):
#   shape           regime   without GELU   with GELU (what the 1e-6 term leaves)
#   1x8x8x1x4       unit     1.79           0
#   1x8x8x1x4       tiny     1.67           0
#   2x16x8x5x8      unit     2.48           0
#   2x16x8x5x8      tiny     3.07           0
#   1x24x8x683x16   unit     3.18           0.63
#   1x24x8x683x16   tiny     4.52           0
#   1x8x8x12289x4   unit     3.36           0.80
#   1x8x8x12289x4   tiny     4.53           0
#   2x16x8x5x8      offset   0.80           0.78
# Without the GELU the bound has no 1e-6 term (it stands for gelu_grad_f's error), so those rows measure c alone.
MEASURED_C_MAX = 4.53
VJP_C = 2 * MEASURED_C_MAX


def vjp_id(cr):
    return gn_id(cr[0]) + "-" + cr[1]


def vjp_inputs(c, regime):
    """x, da, gy [B, C, F, T], gamma, wide film of a VJP case."""
    B, C, G, Fq, T = c[:5]
    g = torch.Generator().manual_seed(_seed(5, REGIMES.index(regime), B, C, Fq, T))
    x = gn_data(regime, B, C, G, Fq, T)
    da, gy = torch.randn(x.shape, generator=g), torch.randn(x.shape, generator=g)
    gamma, wide = gn_params(B, C)
    return x, da, gy, gamma, wide


def vjp_autograd64(x, da, gy, rbeta, gamma, film, G, gelu):
    """The reference: float64 autograd through the oracle's group_norm_nomean * (film + 1), with F.gelu or without."""
    C = x.shape[1]
    xr = x.double().requires_grad_(True)
    y = UN.group_norm_nomean(xr, gamma.double().view(1, C, 1, 1), groups=G, eps=EPS) * (film.double()[:, :, None, None] + 1)
    gx, = torch.autograd.grad(((F.gelu(y) if gelu else y) * da.double()).sum(), xr)
    return gx if gy is None else gx + rbeta * gy.double()


def vjp_closed64(x, da, gy, rbeta, gamma, film, G, gelu):
    """The header's closed form in float64, and the two sums of magnitudes the bound is made of:
    (gx, t32, tg) with |gx_kernel - gx| <= VJP_C * 2^-24 * t32 + 1e-6 * tg   (tg only with the GELU)."""
    B, C, Fq, T = x.shape
    cg, n = C // G, (C // G) * Fq * T
    ref = gn_ref64(x, gamma, film, G)
    x64, da64 = x.double(), da.double()
    sc = ref["scale"][:, :, None, None]
    du = da64 * gelu_grad64(ref["u"]) if gelu else da64
    grp = lambda t: t.reshape(B, G, -1).sum(-1)                                           # noqa: E731
    per = lambda v: v.repeat_interleave(cg, dim=1)[:, :, None, None]                      # noqa: E731  [B, G] -> [B, C, 1, 1]
    den = (n - 1) * ref["std"] * (ref["std"] + EPS)
    ok = ref["std"] > 0
    safe = torch.where(ok, den, torch.ones_like(den))
    coef = torch.where(ok, grp(du * sc * x64) / safe, torch.zeros_like(den))
    A = torch.where(ok, grp((du * sc * x64).abs()) / safe, torch.zeros_like(den))
    Ada = torch.where(ok, grp((da64 * sc * x64).abs()) / safe, torch.zeros_like(den))
    m = per(ref["mean"])
    gx = sc * du - (x64 - m) * per(coef)
    t32 = (sc * du).abs() + ((x64 - m) * per(coef)).abs() + (x64 - m).abs() * per(A) + per(coef).abs() * m.abs()
    if gy is not None:
        gx = gx + rbeta * gy.double()
        t32 = t32 + (rbeta * gy.double()).abs()
    tg = (sc * da64).abs() + (x64 - m).abs() * per(Ada) if gelu else torch.zeros_like(gx)
    return gx, t32, tg


def vjp_bound(t32, tg):
    return VJP_C * U32 * t32 + GELU_BAR * tg


def vjp_restate32(x, da, gy, rbeta, scale, stats, G, gelu, eps=EPS):
    """gn_bwd_partial + gn_bwd_apply in kernel order on the CPU: float32 terms, S accumulated in float64, the coefficient formed
    in double and rounded.  scale [B, C], stats [B, G, 3]: float32, as the forward stored them."""
    B, C, Fq, T = x.shape
    cg, n = C // G, (C // G) * Fq * T
    sc = scale[:, :, None, None]
    du = da * gelu_grad32(x * sc) if gelu else da
    S1 = ((du.double() * x.double()).sum((2, 3)) * scale.double()).reshape(B, G, cg).sum(-1)
    sd = stats[:, :, 1].double()
    se = sd + float(np.float32(eps))
    coef = torch.where(sd > 0, S1 * se / ((n - 1) * sd * se * se).clamp_min(1e-300), torch.zeros_like(sd)).float()
    per = lambda v: v.repeat_interleave(cg, dim=1)[:, :, None, None]                      # noqa: E731
    o = sc * du - (x - per(stats[:, :, 0])) * per(coef)
    return o if gy is None else o + _f(rbeta) * gy


def _vjp_buffers(k, x, da, gy_mode, gy, scale, stats, S, G):
    B = x.shape[0]
    xg, dg, sg, tg = k.f32("x", x), k.f32("da", da), k.f32("scale", scale), k.f32("stats", stats)
    part = k.f64("part", B * G * S)
    if gy_mode == "alias":
        gx = k.f32("gx", gy)
        gyp = _p(gx)
    else:
        gx = k.f32("gx", n=x.numel())
        gyp = _p(k.f32("gy", gy)) if gy_mode == "separate" else None
    return xg, dg, sg, tg, part, gx, gyp


def gn_bwd_partial(x, da, scale, G, gelu, S=None):
    """babe_gn_bwd_partial(_nogelu): part [B*G, S] float64."""
    from babe_amd._lib import check, lib, stream
    B, C, Fq, T = x.shape
    S = S or gn_splits((C // G) * Fq * T)
    k = Canaried()
    xg, dg, sg, part = k.f32("x", x), k.f32("da", da), k.f32("scale", scale), k.f64("part", B * G * S)
    L = lib()
    fn = L.babe_gn_bwd_partial if gelu else L.babe_gn_bwd_partial_nogelu
    check(fn(_p(xg), _p(dg), _p(sg), _p(part), B, C, G, Fq * T, S, stream()), "gn_bwd_partial")
    k.check(f"gn_bwd_partial {tuple(x.shape)} S={S}")
    return part.mid.view(torch.float64).cpu().reshape(B * G, S)


def gn_bwd(x, da, gy_mode, gy, rbeta, scale, stats, G, gelu, merge=None):
    """partial + apply (babe_gn_bwd_apply, _nogelu, or _merge with merge = (acc, ca, cb)): gx on the CPU.  gy_mode: "none",
    "alias" (gy lives in gx's buffer) or "separate"."""
    from babe_amd._lib import check, lib, stream
    B, C, Fq, T = x.shape
    hw = Fq * T
    S = gn_splits((C // G) * hw)
    k = Canaried()
    xg, dg, sg, tg, part, gx, gyp = _vjp_buffers(k, x, da, gy_mode, gy, scale, stats, S, G)
    L, st = lib(), stream()
    partial = L.babe_gn_bwd_partial if gelu else L.babe_gn_bwd_partial_nogelu
    check(partial(_p(xg), _p(dg), _p(sg), _p(part), B, C, G, hw, S, st), "gn_bwd_partial")
    args = (_p(xg), _p(dg), gyp, _p(sg), _p(tg), _p(part), _p(gx), rbeta, B, C, G, hw, S, EPS, st)
    if merge is not None:
        acc, ca, cb = merge
        check(L.babe_gn_bwd_apply_merge(*args, _p(k.f32("acc", acc)), ca, cb), "gn_bwd_apply_merge")
    else:
        check((L.babe_gn_bwd_apply if gelu else L.babe_gn_bwd_apply_nogelu)(*args), "gn_bwd_apply")
    k.check(f"gn_bwd {tuple(x.shape)} gy={gy_mode} gelu={gelu}")
    return gx.mid.cpu().reshape(x.shape)


def straddle_expected(x, da, scale, G, S):
    """Exact per-split sums of babe_gn_bwd_partial_nogelu in float64: [B*G, S], and whether some split holds parts of two channels."""
    B, C, Fq, T = x.shape
    hw, n = Fq * T, (C // G) * Fq * T
    term = (da.double() * x.double() * scale.double()[:, :, None, None]).reshape(B * G, n)
    rng = split_ranges(n, S)
    want = torch.stack([term[:, b:e].sum(-1) if b < e else torch.zeros(B * G, dtype=torch.float64) for b, e in rng], 1)
    return want, any(b < e and b // hw != (e - 1) // hw for b, e in rng)


# ============================================================================= D. resample
RS_T = (8, 10, 12, 16, 20, 24, 32, 36)
RS_SHAPES = ((1, 1, 1), (2, 3, 3))                # (B, C, F): (B*C, F) = (1, 1) and (6, 3)
RS_ALPHA = (1.0, 0.5, -2.0)
RS_BETA = (0.0, 1.0, 0.25)
# where the operands lie: dense; the input / the output carved one float (4 bytes) into a flat buffer; the output a frequency
# sub-view; babe_resample_res with res a channel slice
RS_LAYOUTS = ("dense", "in+4B", "out+4B", "subview", "res")
RS_FEW = ((1.0, 0.0), (0.5, 1.0), (-2.0, 0.25))   # the (alpha, beta) of every layout but dense (dense: all nine)
RS_SUB = (2, 1)                                   # rows of the wider output before / after the sub-view
RS_INEXACT_T = (8, 12, 36, 64)


def rs_lengths(mode, T):
    """(Tin, Tout) of a mode; T is the forward operator's input length."""
    return (T, T // 2) if mode == 0 else (T, 2 * T) if mode == 1 else (T // 2, T) if mode == 2 else (2 * T, T)


def rs_geometry(layout, mode, B, C, Fq, T):
    """Offsets (floats, from a 16-byte aligned base) and (batch, channel) strides of in, out and res in a layout:
    dict(in_=(off, bs, cs), out=(off, bs, cs, rows of the buffer), res=None or (off, bs, cs))."""
    Tin, Tout = rs_lengths(mode, T)
    g = dict(in_=(0, C * Fq * Tin, Fq * Tin), out=(0, C * Fq * Tout, Fq * Tout, Fq), res=None)
    if layout == "in+4B":
        g["in_"] = (1,) + g["in_"][1:]
    elif layout == "out+4B":
        g["out"] = (1,) + g["out"][1:]
    elif layout == "subview":
        rows = RS_SUB[0] + Fq + RS_SUB[1]
        g["out"] = (RS_SUB[0] * Tout, C * rows * Tout, rows * Tout, rows)
    elif layout == "res":
        g["res"] = (C * Fq * Tout, 2 * C * Fq * Tout, Fq * Tout)
    return g


def rs_variant(mode, T, geo):
    """The launcher's rule restated: "4,1", "4,0" or "1,0" = resample_kernel<V, VI>."""
    Tin, Tout = rs_lengths(mode, T)
    al = lambda v: all(e % 4 == 0 for e in v[:3])                                          # noqa: E731
    v4 = Tout % 4 == 0 and al(geo["out"])
    vin = Tin % 4 == 0 and al(geo["in_"])
    return "4,1" if v4 and vin else "4,0" if v4 else "1,0"


def rs_res_legal(geo):
    """babe_resample_res takes only 16-byte aligned res / out views."""
    return all(e % 4 == 0 for e in geo["res"] + geo["out"][:3])


def rs_runs(mode, T):
    """Every (shape, layout, alpha, beta) of the exact table for one (mode, T)."""
    out = []
    for shape in RS_SHAPES:
        for layout in RS_LAYOUTS:
            pairs = [(a, b) for a in RS_ALPHA for b in RS_BETA] if layout == "dense" else RS_FEW
            out += [(shape, layout, a, b) for a, b in pairs if not (layout == "res" and b == 0.0)]
    return out


def _fir_down(x, h):
    B, C, Fq, T = x.shape
    xp = F.pad(x.reshape(B * C * Fq, 1, T), (3, 3), mode="reflect")
    return F.conv1d(xp, h.view(1, 1, 8), stride=2).reshape(B, C, Fq, -1)


def _fir_up(x, h):
    B, C, Fq, T = x.shape
    xp = F.pad(x.reshape(B * C * Fq, 1, T), (2, 2), mode="reflect")
    return F.conv_transpose1d(xp, h.view(1, 1, 8), stride=2, padding=7).reshape(B, C, Fq, -1)


def resample64(mode, x, T, absolute=False):
    """float64 reference of a mode on x [B, C, F, Tin]: the oracle's operators (reflect padding, CUBIC taps) and, for modes 2 / 3,
    their adjoints by autograd.  absolute: the same operator with |taps| on |x|: sum_k |h_k x_k| of every output."""
    h = torch.tensor(UN.CUBIC, dtype=torch.float64)
    x = x.double()
    if absolute:
        h, x = h.abs(), x.abs()
    fwd = _fir_down if mode in (0, 2) else _fir_up
    if mode in (0, 1):
        return fwd(x, h)
    z = torch.zeros(x.shape[:3] + (T,), dtype=torch.float64, requires_grad=True)
    g, = torch.autograd.grad((fwd(z, h) * x).sum(), z)
    return g


def rs_inputs(mode, shape, T, integers=True):
    """x [B, C, F, Tin] and res [B, C, F, Tout]: integers in [-1024, 1024], or randn."""
    B, C, Fq = shape
    Tin, Tout = rs_lengths(mode, T)
    g = torch.Generator().manual_seed(_seed(3, mode, B * C, Fq, T, int(integers)))
    if integers:
        return (torch.randint(-1024, 1025, (B, C, Fq, Tin), generator=g).float(),
                torch.randint(-1024, 1025, (B, C, Fq, Tout), generator=g).float())
    return torch.randn(B, C, Fq, Tin, generator=g), torch.randn(B, C, Fq, Tout, generator=g)


def rs_bits_needed(alpha, beta, xmax=1024):
    """Bits a float32 must hold for EVERY partial sum of alpha * sum_k h_k x_k + beta * res to be exact with |x|, |res| <= xmax,
    taps k / 256 and power-of-two alpha, beta: all terms are multiples of q, and the sum of their magnitudes (the border folds at
    most double the taps' sum) stays below 2^bits * q."""
    habs = sum(abs(v) for v in UN.CUBIC)
    assert all(v * 256 == int(v * 256) for v in UN.CUBIC)
    for v in (alpha, beta):
        assert v == 0 or math.log2(abs(v)) == int(math.log2(abs(v)))
    q = min([abs(alpha) / 256] + ([abs(beta)] if beta else []) + [1 / 256])
    return math.ceil(math.log2((max(abs(alpha), 1.0) * 2 * habs * xmax + abs(beta) * xmax) / q))


def rs_inexact_bound(mode, x, res, T, alpha, beta):
    b = abs(alpha) * resample64(mode, x, T, absolute=True)
    return 10 * U32 * (b + (abs(beta) * res.double().abs() if beta else 0.0))


def resample_call(mode, x, res, T, alpha, beta, layout, out_fill=NAN):
    """One babe_resample / babe_resample_res call in a layout.  With beta = 0 the output buffer is all `out_fill`; otherwise it
    holds res (for layout "res": NaN, res is a channel slice of another buffer whose other half is NaN).
    Returns (rc, out [B, C, F, Tout] on the CPU, the output buffer's rows outside the view or None)."""
    from babe_amd._lib import lib, stream
    B, C, Fq, Tin = x.shape
    Tout = rs_lengths(mode, T)[1]
    geo = rs_geometry(layout, mode, B, C, Fq, T)
    k = Canaried()
    ioff, ibs, ics = geo["in_"]
    xin = k.f32("in", n=ioff + x.numel())
    xin.mid[ioff:].copy_(x.reshape(-1))
    ooff, obs, ocs, rows = geo["out"]
    out = k.f32("out", n=(1 if layout == "out+4B" else 0) + B * C * rows * Tout, fill=out_fill)
    if layout == "subview":
        view = out.mid.reshape(B, C, rows, Tout)[:, :, RS_SUB[0]:RS_SUB[0] + Fq, :]
    else:
        view = out.mid[ooff:].reshape(B, C, Fq, Tout)
    if beta != 0.0 and layout != "res":
        view.copy_(res)
    L, st = lib(), stream()
    if layout == "res":
        roff, rbs, rcs = geo["res"]
        cat = k.f32("res", n=B * 2 * C * Fq * Tout)
        cat.mid.reshape(B, 2 * C, Fq, Tout)[:, C:].copy_(res)
        rc = L.babe_resample_res(_p(xin, ioff), ibs, ics, _p(cat, roff), rbs, rcs, _p(out, ooff), obs, ocs, B, C, Fq, T, mode,
                                 alpha, beta, st)
    else:
        rc = L.babe_resample(_p(xin, ioff), ibs, ics, _p(out, ooff), obs, ocs, B, C, Fq, T, mode, alpha, beta, st)
    k.check(f"resample mode {mode} T={T} {layout}")
    outside = None
    if layout == "subview":
        full = out.mid.cpu().reshape(B, C, rows, Tout)
        outside = torch.cat([full[:, :, :RS_SUB[0]], full[:, :, RS_SUB[0] + Fq:]], 2)
    return rc, view.cpu().clone(), outside


# ============================================================================= E. element-wise kernels
# axpby4d: (name, B, C, F, T, in (off, extra floats per plane), out (off, extra floats per plane), kernel variant, what it reaches)
# a plane stride is F*T + extra; off: floats from the aligned base
AXPBY_CASES = [
    ("vector", 2, 3, 4, 8, (0, 0), (0, 0), 4, "the 16-byte variant, dense"),
    ("odd", 2, 3, 3, 5, (0, 0), (0, 0), 1, "scalar variant: F*T odd"),
    ("unaligned", 2, 3, 4, 8, (1, 0), (0, 0), 1, "scalar variant: input pointer 4 bytes off"),
    ("stride", 2, 3, 4, 8, (0, 0), (0, 2), 1, "scalar variant: output strides % 4 != 0"),
    ("views", 2, 3, 4, 8, (16, 24), (8, 40), 4, "both sides frequency sub-views (aligned): 16-byte variant"),
    ("big-vector", 1, 2, 1, 65540, (0, 0), (0, 8), 4, "16385 float4 per plane: the 64-block grid-stride loop takes a second turn"),
    ("big-scalar", 1, 2, 1, 16385, (0, 0), (0, 3), 1, "16385 floats per plane, scalar: second turn"),
]
AXPBY_EXACT = ((1.0, 0.0), (0.5, 0.0), (-2.0, 1.0), (0.25, 0.5))
AXPBY_GENERAL = ((1.0 / math.sqrt(2.0), 0.0), (0.3, -1.7), (1.0 / math.sqrt(2.0), 1.0))
AXPBY2_CASES = [("dense", 2, 3, 4, 8, 0), ("out-subview", 2, 3, 4, 8, 24), ("big", 1, 2, 1, 65540, 8)]      # last: extra floats per out plane
AXPBY2_FACTORS = ((1.0 / math.sqrt(2.0), 1.0 / math.sqrt(2.0)), (0.3, -1.7))
FILL_CASES = [(1, 1), (3, 341), (1, 65537)]       # (F, T): F*T = 1, 1023, 65537
FILL_VALUES = (0.0, -1.5)
LINEAR_CASES = [(1, 1, 1), (3, 63, 5), (2, 65, 4)]        # (B, K, J)


def axpby_variant(B, C, Fq, T, inl, outl):
    """babe_axpby4d's rule restated: 4 = the 16-byte variant, 1 = scalar."""
    n = Fq * T
    al = lambda l: l[0] % 4 == 0 and (n + l[1]) % 4 == 0                                  # noqa: E731  (bs = C * cs)
    return 4 if n % 4 == 0 and al(inl) and al(outl) else 1


def axpby_blocks(n, V):
    """(workgroups, elements one sweep of the grid covers): more than one sweep = a second turn of the grid-stride loop."""
    bx = min(-(-(n // 4 if V == 4 else n) // 256), 64)
    return bx, bx * 256 * V


def _planes(k, name, t, off, extra, fill):
    """t [B, C, F, T] laid out in a Guarded buffer at float offset `off` with plane stride F*T + extra; the gaps hold `fill`."""
    B, C, Fq, T = t.shape
    cs = Fq * T + extra
    gd = k.f32(name, n=off + B * C * cs, fill=fill)
    v = gd.mid[off:].reshape(B * C, cs)
    v[:, :Fq * T].copy_(t.reshape(B * C, -1))
    return gd, v, cs


def axpby_call(x, y, alpha, beta, inl, outl, gap=7.0):
    """babe_axpby4d: out = alpha x + beta out.  y None (beta = 0): out pre-filled with NaN.  (out [B, C, F, T], gaps intact?)"""
    from babe_amd._lib import check, lib, stream
    B, C, Fq, T = x.shape
    n = Fq * T
    k = Canaried()
    xin, _, ics = _planes(k, "in", x, inl[0], inl[1], NAN)
    out, ov, ocs = _planes(k, "out", y if y is not None else torch.full_like(x, NAN), outl[0], outl[1], gap)
    check(lib().babe_axpby4d(_p(xin, inl[0]), C * ics, ics, _p(out, outl[0]), C * ocs, ocs, B, C, Fq, T, alpha, beta, stream()), "axpby4d")
    k.check(f"axpby4d {tuple(x.shape)}")
    ov = ov.cpu()
    head = out.mid[:outl[0]].cpu()
    intact = bool((ov[:, n:] == gap).all()) and bool((head == gap).all())
    return ov[:, :n].reshape(x.shape).clone(), intact


def axpby2_call(x, y, alpha, beta, extra, gap=7.0):
    """babe_axpby2_4d into a NaN-filled out with plane stride F*T + extra."""
    from babe_amd._lib import check, lib, stream
    B, C, Fq, T = x.shape
    n = Fq * T
    k = Canaried()
    xin, yin = k.f32("x", x), k.f32("y", y)
    out, ov, ocs = _planes(k, "out", torch.full_like(x, NAN), 0, extra, gap)
    check(lib().babe_axpby2_4d(_p(xin), C * n, n, _p(yin), C * n, n, _p(out), C * ocs, ocs, B, C, Fq, T, alpha, beta, stream()), "axpby2_4d")
    k.check(f"axpby2_4d {tuple(x.shape)}")
    ov = ov.cpu()
    return ov[:, :n].reshape(x.shape).clone(), bool((ov[:, n:] == gap).all())


def fill_call(Fq, T, value, B=2, C=3, old=7.0):
    """babe_fill4d on rows 1 .. 1 + F of a [B, C, F + extra, T] buffer holding `old`: the whole buffer on the CPU and the row count."""
    from babe_amd._lib import check, lib, stream
    rows = Fq + (2 if Fq * T < 60000 else 1)
    k = Canaried()
    buf = k.f32("out", n=B * C * rows * T, fill=old)
    check(lib().babe_fill4d(_p(buf, T), C * rows * T, rows * T, B, C, Fq, T, value, stream()), "fill4d")
    k.check(f"fill4d F={Fq} T={T}")
    return buf.mid.cpu().reshape(B, C, rows, T), rows


def linear_inputs(B, K, J):
    g = torch.Generator().manual_seed(_seed(9, B, K, J))
    return torch.randn(B, K, generator=g), torch.randn(J, K, generator=g), torch.randn(J, generator=g)


def linear_ref64(x, W, bias, relu):
    """(reference, bound): |err| <= (ceil(K / 64) + 8) * 2^-24 * (sum_k |x w| + |b|) - a lane adds ceil(K / 64) products, the wave
    sum adds 6 levels, the bias one more, one to spare; relu is 1-Lipschitz."""
    K = x.shape[1]
    y = x.double() @ W.double().t()
    mag = x.double().abs() @ W.double().abs().t()
    if bias is not None:
        y, mag = y + bias.double(), mag + bias.double().abs()
    return (y.clamp_min(0) if relu else y), (-(-K // 64) + 8) * U32 * mag


def linear_call(x, W, bias, relu):
    from babe_amd._lib import check, lib, stream
    B, K = x.shape
    J = W.shape[0]
    k = Canaried()
    xg, wg, out = k.f32("x", x), k.f32("W", W), k.f32("out", n=B * J)
    bp = _p(k.f32("bias", bias)) if bias is not None else None
    check(lib().babe_linear(_p(xg), _p(wg), bp, _p(out), B, K, J, int(relu), stream()), "linear")
    k.check(f"linear {B}x{K}x{J}")
    return out.mid.cpu().reshape(B, J)
