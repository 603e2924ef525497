"""The streaming kernels of the UNet layer path element by element against float64 references: GroupNorm / FiLM / GELU forward and
input-VJP (csrc/norm.hip), the resamplers and their adjoints (csrc/resample.hip), and the copy / add / fill / linear kernels of
csrc/misc.hip - at the shapes, split counts, data regimes, alignments and strides where they can go wrong.  Cases, references and
bounds: tests/layer_cases.py, pinned on the CPU by tests/test_layer_cases_cpu.py.  Needs a MI355X.

Every direct C-ABI call runs on `Guarded` buffers: inputs between NaN canaries, outputs pre-filled with NaN, canaries checked
after the call.  Where the arithmetic allows it the expectation is exact (small integers, power-of-two factors): a dropped,
duplicated or misplaced element fails an equality.  Bounds are per element and derived in tests/layer_cases.py.

Largest figures measured on a MI355X over every case of this file (each test prints its own as `LAYER_EDGE ...`):
  quantity                                        measured    bound
  mean, std of the statistics                     0.50 ulp    1 ulp
  scale                                           2.81 ulp    4 ulp
  a = gelu(x scale), share of 1e-6 + 8 u |u|      0.38        1
  gelu_grad_f, absolute                           2.9e-7      1e-6
  GroupNorm VJP per element, share of its bound   0.45        1
  GroupNorm VJP group sums with GELU, share       0.06        1
  resample at alpha = 1/sqrt2, share of 10 u      0.33        1
"""
import math

import pytest
import torch

from tests import layer_cases as lc

pytestmark = pytest.mark.gpu

GN_IDS = [lc.gn_id(c) for c in lc.GN_CASES]
_FWD = {}


def _forward(c, regime):
    """Inputs, float64 reference and the three forms' results of one (row, regime); computed once and shared, never modified."""
    key = (lc.gn_id(c), regime)
    if key not in _FWD:
        B, C, G, Fq, T = c[:5]
        x = lc.gn_data(regime, B, C, G, Fq, T)
        gamma, wide = lc.gn_params(B, C)
        ref = lc.gn_ref64(x, gamma, lc.film_of(wide, C), G)
        _FWD[key] = (x, gamma, wide, ref, {f: lc.gn_forward(f, x, gamma, wide, G) for f in lc.FORMS3})
    return _FWD[key]


def _rec(what, value):
    print(f"LAYER_EDGE {what} {value:.3e}")
    return value


# ----------------------------------------------------------------------------- A. GroupNorm statistics and scale; B. forward bound
def test_split_rule_is_the_librarys():
    from babe_amd._lib import lib
    L = lib()
    for n in [4, 40, 80, 16383, 16384, 32767, 32768, 32784, 49156, 655360, 1 << 20, (1 << 20) + 4, 1 << 24] + [c[5] for c in lc.GN_CASES]:
        assert lc.gn_splits(n) == int(L.babe_gn_splits(n)), n
    for c in lc.GN_CASES:
        assert c[6] == int(L.babe_gn_splits(c[5]))


@pytest.mark.parametrize("regime", lc.REGIMES)
@pytest.mark.parametrize("c", lc.GN_CASES, ids=GN_IDS)
def test_gn_forward_three_forms(c, regime):
    B, C, G, Fq, T, n, S, _ = c
    x, gamma, wide, ref, got = _forward(c, regime)
    two = got["two"]
    # bit identity of the three forms: partial sums, statistics, scale and output
    for f in ("one", "folded"):
        for k in ("part", "stats", "scale", "a"):
            assert torch.equal(got[f][k].view(torch.int32), two[k].view(torch.int32)), (f, k)
    assert not bool(torch.isnan(two["part"]).any()) and not bool(torch.isnan(two["a"]).any())
    xg = x.double().reshape(B * G, -1)
    if regime in ("integers", "offset"):
        assert torch.equal(two["part"][:, :, 0].sum(1), xg.sum(1)) and torch.equal(two["part"][:, :, 1].sum(1), (xg * xg).sum(1))
        for s, (b, e) in enumerate(lc.split_ranges(n, S)):                                # ... and split by split
            assert torch.equal(two["part"][:, s, 0], xg[:, b:e].sum(1)) and torch.equal(two["part"][:, s, 1], (xg[:, b:e] ** 2).sum(1))
    st = two["stats"]
    if regime != "constant":
        assert _rec("mean ulp", float(lc.ulps32(st[:, :, 0], ref["mean"]).max())) <= 1
        assert _rec("std ulp", float(lc.ulps32(st[:, :, 1], ref["std"]).max())) <= 1
        assert _rec("scale ulp", float(lc.ulps32(two["scale"], ref["scale"]).max())) <= 4
        assert torch.equal(st[:, :, 2], 1.0 / (st[:, :, 1] + torch.tensor(lc.EPS, dtype=torch.float32)))
        err = (two["a"].double() - ref["a"]).abs()
        _rec("a share", float((err / lc.fwd_bound(ref["u"])).max()))
        assert bool((err <= lc.fwd_bound(ref["u"])).all())
        return
    # constant: std == 0 exactly and r == 1 / eps in float32; a finite, gelu of the exact product within the bound; zero group: a == 0
    flat = st.reshape(B * G, 3)
    eps32 = torch.tensor(lc.EPS, dtype=torch.float32)
    assert float(flat[0, 0]) == 0.5 and float(flat[0, 1]) == 0.0 and float(flat[0, 2]) == float(torch.tensor(1.0) / eps32)
    assert bool(torch.isfinite(two["a"]).all()) and bool(torch.isfinite(two["scale"]).all())
    cg = C // G
    film = lc.film_of(wide, C)
    sc64 = gamma.double()[None, :] * (film.double() + 1) / lc.EPS                         # std = 0: scale = gamma (film + 1) / eps
    u0 = 0.5 * sc64[0, :cg][:, None].expand(cg, Fq * T).reshape(-1)
    a0 = two["a"].reshape(B * G, -1)[0].double()
    assert bool(((a0 - lc.gelu64(u0)).abs() <= lc.fwd_bound(u0)).all())
    assert _rec("constant scale ulp", float(lc.ulps32(two["scale"][0, :cg], sc64[0, :cg]).max())) <= 4
    if B * G > 1:
        assert float(flat[1, 0]) == 0.0 and float(flat[1, 1]) == 0.0
        assert float(two["a"].reshape(B * G, -1)[1].abs().max()) == 0.0
        # the other groups are ordinary data: the bounds of every other regime
        rest = slice(2, None)
        assert float(lc.ulps32(flat[rest, 1], ref["std"].reshape(-1)[rest]).max()) <= 1
        err = (two["a"].double() - ref["a"]).abs().reshape(B * G, -1)[rest]
        assert bool((err <= lc.fwd_bound(ref["u"]).reshape(B * G, -1)[rest]).all())


@pytest.mark.parametrize("c", [lc.GN_CASES[1], lc.GN_CASES[3]], ids=[GN_IDS[1], GN_IDS[3]])
def test_ops_forms_are_the_direct_calls(c, monkeypatch):
    """babe_amd.ops under each FORMS setting gives the bits of the direct calls (film a column slice there too)."""
    from babe_amd import ops
    from babe_amd.forms import FORMS
    B, C, G, Fq, T = c[:5]
    x, gamma, wide, _, got = _forward(c, "unit")
    xc, gc, film = x.cuda(), gamma.cuda(), lc.film_of(wide.cuda(), C)
    for fused in (False, True):
        monkeypatch.setattr(FORMS, "gn_fused", fused)
        st, sc = ops.gn_scale(xc, gc, film, G=G, eps=lc.EPS)
        assert torch.equal(st.cpu(), got["two"]["stats"]) and torch.equal(sc.cpu(), got["two"]["scale"])
    for fin in (False, True):
        monkeypatch.setattr(FORMS, "gelu_fin", fin)
        a = torch.full_like(xc, lc.NAN)
        st, sc = ops.gn_scale_gelu(xc, gc, film, a, G=G, eps=lc.EPS)
        assert torch.equal(st.cpu(), got["two"]["stats"]) and torch.equal(sc.cpu(), got["two"]["scale"]) and torch.equal(a.cpu(), got["two"]["a"])


@pytest.mark.parametrize("S", lc.PART_SPLITS)
def test_gn_partial_and_finalize_with_a_chosen_split_count(S):
    """n = 40: S > n / 4 leaves splits with beg >= end, which must store exact zeros (part is NaN before the call); finalize adds
    S > 32 entries in two rounds."""
    B, C, G, Fq, T = lc.PART_SHAPE
    n = (C // G) * Fq * T
    gamma, wide = lc.gn_params(B, C)
    for regime in ("integers", "unit"):
        x = lc.gn_data(regime, B, C, G, Fq, T)
        part, stats, scale = lc.gn_partial_finalize(x, gamma, wide, G, S)
        xg = x.double().reshape(B * G, n)
        for s, (b, e) in enumerate(lc.split_ranges(n, S)):
            if b >= e:
                assert torch.equal(part[:, s], torch.zeros(B * G, 2, dtype=torch.float64)), s
            elif regime == "integers":
                assert torch.equal(part[:, s, 0], xg[:, b:e].sum(1)) and torch.equal(part[:, s, 1], (xg[:, b:e] ** 2).sum(1)), s
        assert not bool(torch.isnan(part).any())
        ref = lc.gn_ref64(x, gamma, lc.film_of(wide, C), G)
        assert float(lc.ulps32(stats[:, :, 0], ref["mean"]).max()) <= 1 and float(lc.ulps32(stats[:, :, 1], ref["std"]).max()) <= 1
        assert float(lc.ulps32(scale, ref["scale"]).max()) <= 4


def test_gelu_derivative_alone():
    """gelu_grad_f isolated: hand-made stats with std = 0 make the kernel's coefficient 0, scale = 1 and da = 1 leave gx = gelu'(x)."""
    from babe_amd import ops
    x = torch.linspace(-8, 8, 8 * 8 * 4096).reshape(1, 8, 8, 4096).contiguous()
    stats = torch.zeros(1, 8, 3)
    stats[:, :, 2] = 1.0 / lc.EPS
    gx = torch.full_like(x, lc.NAN).cuda()
    ops.gn_bwd(x.cuda(), torch.ones_like(x).cuda(), None, torch.ones(1, 8).cuda(), stats.cuda(), gx, 0.0)
    err = (gx.cpu().double() - lc.gelu_grad64(x)).abs()
    assert _rec("gelu' abs", float(err.max())) <= lc.GELU_BAR


@pytest.mark.parametrize("B,C,Fq,T,_", lc.UNITS_CASES, ids=[f"T{c[3]}" for c in lc.UNITS_CASES])
def test_scale_gelu_units(B, C, Fq, T, _):
    x = lc.gn_data("unit", B, C, 8, Fq, T)
    scale = 0.5 + torch.rand(B, C, generator=torch.Generator().manual_seed(T))
    a, buf, nu = lc.units_call(x, scale)
    assert nu == B * (C // 8) * Fq * 4 * (T // 4 + 1) * 8 and buf.numel() > nu
    err = (a.double() - lc.gelu64(x.double() * scale.double()[:, :, None, None])).abs()
    assert bool((err <= lc.fwd_bound(x.double() * scale.double()[:, :, None, None])).all())
    want = lc.units_expected(a)
    assert torch.equal(buf[:nu].reshape(want.shape), want)                                # values, and zeros at t = -1 and t >= T
    assert bool((buf[nu:] == lc.BF16_NAN).all())                                          # nothing beyond


# ----------------------------------------------------------------------------- C. GroupNorm input-VJP
@pytest.mark.parametrize("gelu", [True, False], ids=["gelu", "nogelu"])
@pytest.mark.parametrize("cr", lc.VJP_CASES, ids=[lc.vjp_id(cr) for cr in lc.VJP_CASES])
def test_gn_vjp_per_element(cr, gelu):
    c, regime = cr
    B, C, G, Fq, T = c[:5]
    x, da, gy, gamma, wide = lc.vjp_inputs(c, regime)
    film = lc.film_of(wide, C)
    fwd = lc.gn_forward("two", x, gamma, wide, G)
    for gm, rbeta in lc.VJP_VARIANTS:
        g = None if gm == "none" else gy
        ref = lc.vjp_autograd64(x, da, g, rbeta, gamma, film, G, gelu)
        _, t32, tg = lc.vjp_closed64(x, da, g, rbeta, gamma, film, G, gelu)
        got = lc.gn_bwd(x, da, gm, g, rbeta, fwd["scale"], fwd["stats"], G, gelu)
        err = (got.double() - ref).abs()
        _rec(f"vjp share {gm} {rbeta}", float((err / lc.vjp_bound(t32, tg)).max()))
        assert bool((err <= lc.vjp_bound(t32, tg)).all()), (gm, rbeta)


@pytest.mark.parametrize("c", lc.GN_CASES[:4], ids=GN_IDS[:4])
def test_gn_vjp_partial_sums(c):
    """Exact with integer x, da and power-of-two scales (split by split: the channel-by-channel loop of a split that holds parts of
    two channels); with the GELU inside (4 * 2^-24 + 1.13 * 1e-6) * sum |da scale x|."""
    B, C, G, Fq, T, n, S = c[:7]
    x, da = lc.gn_data("integers", B, C, G, Fq, T), lc.gn_data("integers", B, C, G, Fq, T).flip(3)
    gamma, _ = lc.gn_params(B, C, pow2=True)
    scale = gamma[None, :].repeat(B, 1).contiguous()
    runs = [S] + ([1, 3, 7] if lc.gn_id(c) == "2x16x8x5x8" else [])                       # n = 80: caller-chosen splits across channels
    for s_run in runs:
        want, _ = lc.straddle_expected(x, da, scale, G, s_run)
        got = lc.gn_bwd_partial(x, da, scale, G, gelu=False, S=s_run)
        assert torch.equal(got.sum(1), want.sum(1)), s_run
        assert torch.equal(got, want), s_run
    for regime in ("unit", "tiny"):
        x, da, _, gamma, wide = lc.vjp_inputs(c, regime)
        sc = lc.gn_forward("two", x, gamma, wide, G)["scale"]
        s4 = sc.double()[:, :, None, None]
        got = lc.gn_bwd_partial(x, da, sc, G, gelu=True).sum(1)
        ref = (da.double() * lc.gelu_grad64(x.double() * s4) * x.double() * s4).reshape(B * G, -1).sum(-1)
        bar = (4 * lc.U32 + lc.GELU_GRAD_MAX * lc.GELU_BAR) * (da.double() * s4 * x.double()).abs().reshape(B * G, -1).sum(-1)
        _rec(f"S_g share {regime}", float(((got - ref).abs() / bar).max()))
        assert bool(((got - ref).abs() <= bar).all())


@pytest.mark.parametrize("c", lc.GN_CASES[:4], ids=GN_IDS[:4])
def test_gn_vjp_merged_tail_is_the_stated_rounding(c):
    """babe_gn_bwd_apply_merge == float32 fl(fl(ca acc) + fl(cb gx)) of the unmerged result, formed by torch on the CPU."""
    B, C, G, Fq, T = c[:5]
    x, da, gy, gamma, wide = lc.vjp_inputs(c, "unit")
    acc = torch.randn(x.shape, generator=torch.Generator().manual_seed(Fq))
    fwd = lc.gn_forward("two", x, gamma, wide, G)
    gx = lc.gn_bwd(x, da, "separate", gy, 0.5, fwd["scale"], fwd["stats"], G, True)
    for ca, cb in ((1.0 / math.sqrt(2.0), 1.0 / math.sqrt(2.0)), (0.3, -1.7)):
        got = lc.gn_bwd(x, da, "separate", gy, 0.5, fwd["scale"], fwd["stats"], G, True, merge=(acc, ca, cb))
        want = torch.tensor(ca, dtype=torch.float32) * acc + torch.tensor(cb, dtype=torch.float32) * gx
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (ca, cb)


@pytest.mark.parametrize("c", lc.GN_CASES[1:3], ids=GN_IDS[1:3])
def test_gn_vjp_of_constant_groups_is_finite(c):
    B, C, G, Fq, T = c[:5]
    x = lc.gn_data("constant", B, C, G, Fq, T)
    _, da, gy, gamma, wide = lc.vjp_inputs(c, "unit")
    fwd = lc.gn_forward("two", x, gamma, wide, G)
    for gelu in (True, False):
        got = lc.gn_bwd(x, da, "separate", gy, 0.5, fwd["scale"], fwd["stats"], G, gelu)
        assert bool(torch.isfinite(got).all()), gelu


# ----------------------------------------------------------------------------- D. resample
@pytest.mark.parametrize("T", lc.RS_T)
@pytest.mark.parametrize("mode", range(4))
def test_resample_exact(mode, T):
    """Integer inputs, power-of-two alpha / beta: torch.equal with the float64 oracle, in every layout of the table."""
    for shape in lc.RS_SHAPES:
        x, res = lc.rs_inputs(mode, shape, T)
        R = lc.resample64(mode, x, T)
        for shp, layout, alpha, beta in lc.rs_runs(mode, T):
            if shp != shape:
                continue
            geo = lc.rs_geometry(layout, mode, shape[0], shape[1], shape[2], T)
            legal = layout != "res" or lc.rs_res_legal(geo)
            rc, out, outside = lc.resample_call(mode, x, res, T, alpha, beta, layout)
            what = (shape, layout, alpha, beta, lc.rs_variant(mode, T, geo))
            if not legal:                                                                 # refused, nothing written
                assert rc != 0 and bool(torch.isnan(out).all()), what
                continue
            assert rc == 0, what
            want = alpha * R + (beta * res.double() if beta else 0.0)
            assert torch.equal(out.double(), want), what
            if outside is not None:                                                       # the rows around a sub-view stay NaN
                assert bool(torch.isnan(outside).all()), what


@pytest.mark.parametrize("T", lc.RS_INEXACT_T)
@pytest.mark.parametrize("mode", range(4))
def test_resample_workload_alpha(mode, T):
    alpha = 1.0 / math.sqrt(2.0)
    x, res = lc.rs_inputs(mode, (2, 3, 3), T, integers=False)
    R = lc.resample64(mode, x, T)
    a32 = float(torch.tensor(alpha, dtype=torch.float32))
    for layout, beta in (("dense", 0.0), ("dense", 1.0), ("res", 1.0), ("in+4B", 1.0)):
        geo = lc.rs_geometry(layout, mode, 2, 3, 3, T)
        if layout == "res" and not lc.rs_res_legal(geo):
            continue
        rc, out, _ = lc.resample_call(mode, x, res, T, alpha, beta, layout)
        assert rc == 0
        err = (out.double() - (a32 * R + beta * res.double())).abs()
        bound = lc.rs_inexact_bound(mode, x, res, T, alpha, beta)
        _rec(f"resample share {layout}", float((err / bound).max()))
        assert bool((err <= bound).all()), (layout, beta)


# ----------------------------------------------------------------------------- E. element-wise kernels
@pytest.mark.parametrize("case", lc.AXPBY_CASES, ids=[c[0] for c in lc.AXPBY_CASES])
def test_axpby4d(case):
    name, B, C, Fq, T, inl, outl, V, _ = case
    g = torch.Generator().manual_seed(len(name) + T)
    xi = torch.randint(-512, 513, (B, C, Fq, T), generator=g).float()
    yi = torch.randint(-512, 513, (B, C, Fq, T), generator=g).float()
    for alpha, beta in lc.AXPBY_EXACT:
        out, intact = lc.axpby_call(xi, yi if beta else None, alpha, beta, inl, outl)
        assert intact and torch.equal(out.double(), alpha * xi.double() + (beta * yi.double() if beta else 0.0)), (alpha, beta)
    x, y = torch.randn(B, C, Fq, T, generator=g), torch.randn(B, C, Fq, T, generator=g)
    for alpha, beta in lc.AXPBY_GENERAL:
        a32, b32 = (float(torch.tensor(v, dtype=torch.float32)) for v in (alpha, beta))
        out, intact = lc.axpby_call(x, y if beta else None, alpha, beta, inl, outl)
        ax, by = a32 * x.double(), (b32 * y.double() if beta else torch.zeros_like(x, dtype=torch.float64))
        assert intact and bool(((out.double() - (ax + by)).abs() <= 2 * lc.U32 * (ax.abs() + by.abs())).all()), (alpha, beta)


@pytest.mark.parametrize("name,B,C,Fq,T,extra", lc.AXPBY2_CASES, ids=[c[0] for c in lc.AXPBY2_CASES])
def test_axpby2_is_torchs_float32_two_products_and_a_sum(name, B, C, Fq, T, extra):
    g = torch.Generator().manual_seed(T + extra)
    x, y = torch.randn(B, C, Fq, T, generator=g), torch.randn(B, C, Fq, T, generator=g)
    for alpha, beta in lc.AXPBY2_FACTORS:
        out, intact = lc.axpby2_call(x, y, alpha, beta, extra)
        want = (torch.tensor(alpha, dtype=torch.float32) * x) + (torch.tensor(beta, dtype=torch.float32) * y)
        assert intact and torch.equal(out.view(torch.int32), want.view(torch.int32)), (alpha, beta)


@pytest.mark.parametrize("value", lc.FILL_VALUES)
@pytest.mark.parametrize("Fq,T", lc.FILL_CASES, ids=[f"{f * t}" for f, t in lc.FILL_CASES])
def test_fill4d(Fq, T, value):
    buf, rows = lc.fill_call(Fq, T, value)
    assert torch.equal(buf[:, :, 1:1 + Fq], torch.full((2, 3, Fq, T), value))
    assert bool((buf[:, :, :1] == 7.0).all()) and bool((buf[:, :, 1 + Fq:] == 7.0).all()) and rows > Fq


@pytest.mark.parametrize("B,K,J", lc.LINEAR_CASES)
def test_linear(B, K, J):
    x, W, bias = lc.linear_inputs(B, K, J)
    for b in (bias, None):
        for relu in (False, True):
            ref, bound = lc.linear_ref64(x, W, b, relu)
            got = lc.linear_call(x, W, b, relu)
            assert bool(((got.double() - ref).abs() <= bound).all()), (b is None, relu)
