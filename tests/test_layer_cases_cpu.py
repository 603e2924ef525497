"""The references, bounds and case tables of tests/test_gpu_layer_edges.py (tests/layer_cases.py), pinned without a GPU: the float64
references equal the oracle and autograd, every table row reaches the path its comment names, the exact cases need at most 24
bits, and the kernels' arithmetic restated in float32 on the CPU stays inside every bound."""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import unet as UN
from tests import layer_cases as lc

GN_IDS = [lc.gn_id(c) for c in lc.GN_CASES]


# ----------------------------------------------------------------------------- A. GroupNorm statistics and scale
@pytest.mark.parametrize("c", lc.GN_CASES, ids=GN_IDS)
def test_gn_table_claims(c):
    B, C, G, Fq, T, n, S, _ = c
    assert C % G == 0 and G <= 64 and (Fq * T) % 4 == 0
    assert n == (C // G) * Fq * T and S == lc.gn_splits(n) and B * C * Fq * T <= 1 << 20
    rng = lc.split_ranges(n, S)
    assert rng[0][0] == 0 and rng[-1][1] == n and all(a[1] == b[0] for a, b in zip(rng, rng[1:])) and all(b < e for b, e in rng)


def test_gn_table_reaches_what_it_names():
    by = {lc.gn_id(c): c for c in lc.GN_CASES}
    assert lc.gn_chunk(4, 1) == 4                                                         # one float4: nv = 1 < 4 * 256, the tail loop
    hw, n = 683 * 16, 32784
    assert by["1x24x8x683x16"][5] == n and lc.gn_chunk(n, 2) == 16392 and hw < 16392 < 2 * hw          # inside the middle channel
    n = by["1x8x8x12289x4"][5]
    assert lc.gn_chunk(n, 3) == 16388 and lc.split_ranges(n, 3)[-1] == (32776, 49156) and 49156 - 32776 == 16380
    assert lc.gn_splits(655360) == 40 and 32 < 40 < 64                                    # lanes 0..7 add two entries, 8..31 one
    assert lc.gn_splits(1 << 20) == 64 and lc.gn_splits((1 << 20) + 16384) == 64          # the clamp
    assert [lc.gn_splits(v) for v in (4, 16383, 16384, 32767, 32768)] == [1, 1, 1, 1, 2]
    # the unrolled loop of gn_partial_kernel runs only for nv > 3 * 256 float4: rows 3 .. 6 take it, rows 1, 2 only its tail
    assert [lc.gn_chunk(c[5], c[6]) // 4 > 768 for c in lc.GN_CASES] == [False, False, True, True, True, True]


def test_direct_partial_splits_have_empty_chunks_past_n_over_4():
    B, C, G, Fq, T = lc.PART_SHAPE
    n = (C // G) * Fq * T
    assert n == 40
    for S in lc.PART_SPLITS:
        empty = [s for s, (b, e) in enumerate(lc.split_ranges(n, S)) if b >= e]
        assert empty == {1: [], 2: [], 3: [], 7: [5, 6], 33: list(range(10, 33)), 64: list(range(10, 64))}[S]
        assert S <= n // 4 or empty
        assert sum(max(e - b, 0) for b, e in lc.split_ranges(n, S)) == n
    assert lc.split_ranges(n, 7) == [(0, 8), (8, 16), (16, 24), (24, 32), (32, 40), (40, 40), (48, 40)]


@pytest.mark.parametrize("c", lc.GN_CASES[:4], ids=GN_IDS[:4])
def test_gn_reference_is_the_oracle(c):
    B, C, G, Fq, T = c[:5]
    x = lc.gn_data("unit", B, C, G, Fq, T)
    gamma, wide = lc.gn_params(B, C)
    film = lc.film_of(wide, C)
    assert wide.shape[1] != C and bool(torch.isnan(wide[:, :lc.FILM_PAD[0]]).all()) and bool(torch.isnan(wide[:, -1]).all())
    want = F.gelu(UN.group_norm_nomean(x.double(), gamma.double().view(1, C, 1, 1), groups=G, eps=lc.EPS) * (film.double()[:, :, None, None] + 1))
    got = lc.gn_ref64(x, gamma, film, G)
    assert float((got["a"] - want).abs().max()) <= 1e-14 * float(want.abs().max())


def test_regimes_are_what_they_say():
    B, C, G, Fq, T = lc.GN_CASES[2][:5]
    n = (C // G) * Fq * T
    x = {r: lc.gn_data(r, B, C, G, Fq, T) for r in lc.REGIMES}
    assert set(x["integers"].unique().tolist()) == {-3.0, -2.0, -1.0, 0.0, 1.0, 2.0, 3.0}
    assert set(x["offset"].unique().tolist()) == {127.0, 128.0, 129.0}
    st = x["tiny"].double().reshape(G, -1).std(-1)
    assert float(st.min()) > 2.5 * lc.EPS and float(st.max()) < 3.5 * lc.EPS
    u = x["unit"].double().reshape(G, -1)
    assert 0.15 < float((u.mean(-1) / u.std(-1)).mean()) < 0.35
    o = x["offset"].double().reshape(G, -1)
    assert float((o.mean(-1) / o.std(-1)).min()) > 100                                    # the mean dominates
    cst = x["constant"].reshape(G, -1)
    assert bool((cst[0] == 0.5).all()) and bool((cst[1] == 0).all()) and float(cst[2].std()) > 1
    # exact sums: every partial sum of x and x^2 is an integer below 2^53
    for r in ("integers", "offset"):
        assert float((x[r].double() ** 2).reshape(G, -1).sum(-1).max()) < 2.0 ** 53 and n * 129 ** 2 < 2 ** 53


@pytest.mark.parametrize("regime", [r for r in lc.REGIMES if r != "constant"])
@pytest.mark.parametrize("c", lc.GN_CASES, ids=GN_IDS)
def test_forward_restatement_stays_inside_the_bounds(c, regime):
    """mean, std within 1 ulp, scale within 4 (largest here: 2.82 - half-ulp relative errors count double in ulps of a reference
    just above a power of two), a within the forward bound (at most 0.52 of it)."""
    B, C, G, Fq, T = c[:5]
    x = lc.gn_data(regime, B, C, G, Fq, T)
    gamma, wide = lc.gn_params(B, C)
    film = lc.film_of(wide, C)
    ref, got = lc.gn_ref64(x, gamma, film, G), lc.gn_restate32(x, gamma, film, G)
    assert float(lc.ulps32(got["stats"][:, :, 0], ref["mean"]).max()) <= 1
    assert float(lc.ulps32(got["stats"][:, :, 1], ref["std"]).max()) <= 1
    assert float(lc.ulps32(got["scale"], ref["scale"]).max()) <= 3
    share = float(((got["a"].double() - ref["a"]).abs() / lc.fwd_bound(ref["u"])).max())
    assert share <= 0.52, share
    if regime in ("integers", "offset"):
        assert torch.equal(got["part"][..., 0], x.double().reshape(B, G, -1).sum(-1))


def test_constant_groups_have_zero_std_and_r_of_one_over_eps():
    for c in lc.GN_CASES:
        B, C, G, Fq, T = c[:5]
        x = lc.gn_data("constant", B, C, G, Fq, T)
        gamma, wide = lc.gn_params(B, C)
        got = lc.gn_restate32(x, gamma, lc.film_of(wide, C), G)
        st = got["stats"].reshape(B * G, 3)
        one_over_eps = float(torch.tensor(1.0) / torch.tensor(lc.EPS, dtype=torch.float32))
        assert float(st[0, 1]) == 0.0 and float(st[0, 2]) == one_over_eps and float(st[0, 0]) == 0.5
        assert bool(torch.isfinite(got["a"]).all())
        if B * G > 1:
            assert float(st[1, 1]) == 0.0 and float(st[1, 0]) == 0.0
            assert float(got["a"].reshape(B * G, -1)[1].abs().max()) == 0.0
    # where eps sits shows on quiet input and not at std = 1
    std = torch.tensor([1.0, 3e-7], dtype=torch.float64)
    forms = torch.stack([1 / (std + lc.EPS), 1 / (std * std + lc.EPS).sqrt(), 1 / std])
    assert float((forms[:, 0] / forms[0, 0] - 1).abs().max()) < 2e-7 and float((forms[1:, 1] / forms[0, 1] - 1).abs().min()) > 0.25


# ----------------------------------------------------------------------------- B. GELU, its derivative, the units
def test_gelu_references_and_restatements():
    u = torch.linspace(-8, 8, 262144, dtype=torch.float64).requires_grad_(True)
    g, = torch.autograd.grad(F.gelu(u).sum(), u)
    assert float((lc.gelu_grad64(u.detach()) - g).abs().max()) < 1e-15
    assert float(lc.gelu_grad64(u.detach()).abs().max()) <= lc.GELU_GRAD_MAX
    u32 = u.detach().float()
    assert float((lc.gelu_grad32(u32).double() - lc.gelu_grad64(u32)).abs().max()) < lc.GELU_BAR / 3
    assert float((lc.gelu32(u32).double() - lc.gelu64(u32)).abs().max()) < lc.GELU_BAR


def test_units_layout():
    for B, C, Fq, T, _ in lc.UNITS_CASES:
        a = torch.arange(1, B * C * Fq * T + 1, dtype=torch.float32).reshape(B, C, Fq, T) / 8
        un = lc.units_expected(a)
        PI = T // 4 + 1
        assert un.shape == (B, C // 8, Fq, 4, PI, 8)
        as_bits = lambda v: int(torch.tensor(v).to(torch.bfloat16).view(torch.int16))          # noqa: E731
        seen = 0
        for b in range(B):
            for ch in range(C):
                for t in range(-1, T + 3):
                    p, j = (t + 1) % 4, (t + 1) // 4
                    want = as_bits(float(a[b, ch, 0, t])) if 0 <= t < T else 0
                    assert int(un[b, ch // 8, 0, p, j, ch % 8]) == want
                    seen += 1
        assert seen == un.numel()                                                         # every entry is one (channel, t) of -1 .. T + 2


# ----------------------------------------------------------------------------- C. GroupNorm input-VJP
@pytest.mark.parametrize("gelu", [True, False], ids=["gelu", "nogelu"])
@pytest.mark.parametrize("cr", lc.VJP_CASES, ids=[lc.vjp_id(cr) for cr in lc.VJP_CASES])
def test_vjp_restatement_stays_inside_the_bound(cr, gelu):
    """The closed form is the autograd reference; the kernel-order float32 restatement needs at most MEASURED_C_MAX, half of VJP_C."""
    c, regime = cr
    B, C, G, Fq, T = c[:5]
    x, da, gy, gamma, wide = lc.vjp_inputs(c, regime)
    film = lc.film_of(wide, C)
    rs = lc.gn_restate32(x, gamma, film, G)
    for gm, rbeta in lc.VJP_VARIANTS:
        g = None if gm == "none" else gy
        ref = lc.vjp_autograd64(x, da, g, rbeta, gamma, film, G, gelu)
        closed, t32, tg = lc.vjp_closed64(x, da, g, rbeta, gamma, film, G, gelu)
        assert float((closed - ref).abs().max()) <= 1e-14 * float(ref.abs().max())
        err = (lc.vjp_restate32(x, da, g, rbeta, rs["scale"], rs["stats"], G, gelu).double() - ref).abs()
        assert bool((err <= lc.vjp_bound(t32, tg)).all())
        need = float(((err - lc.GELU_BAR * tg).clamp_min(0) / (lc.U32 * t32)).max())
        assert need <= lc.MEASURED_C_MAX, need
    assert lc.VJP_C == 2 * lc.MEASURED_C_MAX
    if not gelu:
        assert not bool(tg.any())


@pytest.mark.parametrize("c", lc.GN_CASES[:4], ids=GN_IDS[:4])
def test_vjp_partial_sums(c):
    """Integer data and power-of-two scales give sums exact in float64 in any order; row 3 has a split across two channels; the
    float32 terms of the GELU sums stay inside their bound."""
    B, C, G, Fq, T, n, S = c[:7]
    x, da = lc.gn_data("integers", B, C, G, Fq, T), lc.gn_data("integers", B, C, G, Fq + 0, T).flip(3)
    gamma, _ = lc.gn_params(B, C, pow2=True)
    scale = gamma[None, :].repeat(B, 1)
    want, straddles = lc.straddle_expected(x, da, scale, G, S)
    # a split with parts of more than one channel: row 2 (both channels in its one split) and row 3 (a boundary INSIDE a channel)
    assert want.shape == (B * G, S) and straddles == (lc.gn_id(c) in ("2x16x8x5x8", "1x24x8x683x16"))
    assert (lc.gn_chunk(n, S) % (Fq * T) != 0 and S > 1 and C // G > 1) == (lc.gn_id(c) == "1x24x8x683x16")
    assert torch.equal(want * 4, (want * 4).round()) and float((da.double() * x.double()).abs().sum() * 4) < 2.0 ** 53
    assert torch.equal(want.sum(1), (da.double() * x.double() * scale.double()[:, :, None, None]).reshape(B * G, -1).sum(-1))
    for regime in ("unit", "tiny"):
        x, da, _, gamma, wide = lc.vjp_inputs(c, regime)
        sc = lc.gn_restate32(x, gamma, lc.film_of(wide, C), G)["scale"]
        s4 = sc[:, :, None, None]
        got = ((da * lc.gelu_grad32(x * s4)).double() * x.double() * s4.double()).reshape(B * G, -1).sum(-1)
        ref = (da.double() * lc.gelu_grad64(x.double() * s4.double()) * x.double() * s4.double()).reshape(B * G, -1).sum(-1)
        bar = (4 * lc.U32 + lc.GELU_GRAD_MAX * lc.GELU_BAR) * (da.double() * s4.double() * x.double()).abs().reshape(B * G, -1).sum(-1)
        assert bool(((got - ref).abs() <= bar).all())
    # a caller-chosen S on the n = 80 shape: a split that holds the end of one channel and the start of the next
    B, C, G, Fq, T = lc.GN_CASES[1][:5]
    assert any(b < e and b // 40 != (e - 1) // 40 for b, e in lc.split_ranges(80, 3))


# ----------------------------------------------------------------------------- D. resample
@pytest.mark.parametrize("T", lc.RS_T + (22, 64))
def test_resample_reference_is_the_oracle_and_exact_in_float32(T):
    for shape in lc.RS_SHAPES:
        x, _ = lc.rs_inputs(0, shape, T)
        assert float(x.abs().max()) <= 1024 and torch.equal(x, x.round())
        assert torch.equal(lc.resample64(0, x, T), UN.resample_down(x.double()))
        assert torch.equal(lc.resample64(1, x, T), UN.resample_up(x.double()))
        for mode, fwd in ((2, UN.resample_down), (3, UN.resample_up)):
            gy, _ = lc.rs_inputs(mode, shape, T)
            gx = lc.resample64(mode, gy, T)
            assert gx.shape == x.shape
            assert float((fwd(x.double()) * gy.double()).sum()) == float((x.double() * gx).sum())       # exact: integers / 256
        # the float32 evaluation of the same operators is exact on this data, forward and adjoint
        for mode in range(4):
            xin, _ = lc.rs_inputs(mode, shape, T)
            ref = lc.resample64(mode, xin, T)
            assert torch.equal(ref.float().double(), ref) and torch.equal(ref * 256, (ref * 256).round())
            if mode < 2:
                f32 = (UN.resample_down if mode == 0 else UN.resample_up)(xin)
            else:
                z = torch.zeros(xin.shape[:3] + (T,), requires_grad=True)
                f32, = torch.autograd.grad(((UN.resample_down if mode == 2 else UN.resample_up)(z) * xin).sum(), z)
            assert torch.equal(f32.double(), ref)
            ab = lc.resample64(mode, xin, T, absolute=True)
            assert bool((ab >= ref.abs()).all()) and float(ab.max()) <= 2 * sum(abs(v) for v in UN.CUBIC) * 1024


def test_resample_exact_cases_need_at_most_24_bits():
    for a in lc.RS_ALPHA:
        for b in lc.RS_BETA:
            assert lc.rs_bits_needed(a, b) <= 24, (a, b)
    assert lc.rs_bits_needed(1.0, 2.0 ** -20) > 24                                        # the count does notice a fine quantum


def test_resample_table_reaches_every_launcher_variant():
    reached = {m: {} for m in range(4)}
    for mode in range(4):
        for T in lc.RS_T:
            assert T >= 8 and T % 2 == 0
            for shape, layout, a, b in lc.rs_runs(mode, T):
                geo = lc.rs_geometry(layout, mode, shape[0], shape[1], shape[2], T)
                if layout == "res" and not lc.rs_res_legal(geo):
                    continue
                reached[mode].setdefault(lc.rs_variant(mode, T, geo), set()).add((T, layout))
    for mode in range(4):
        assert set(reached[mode]) == {"4,1", "4,0", "1,0"}, (mode, reached[mode].keys())
    # <4,0> (16-byte output, unaligned input): in modes 0 and 3 only from an input carved 4 bytes into a flat buffer, in modes
    # 1 and 2 also from T = 10 / T = 12, whose source rows are no multiple of 4 long
    for mode in (0, 3):
        assert {l for _, l in reached[mode]["4,0"]} == {"in+4B"}
    assert (10, "dense") in reached[1]["4,0"] and (12, "dense") in reached[2]["4,0"]
    assert 8 in lc.RS_T and 12 in lc.RS_T                   # the launcher's minimum; first, interior and last thread of a row (mode 3)
    # every exact run list has the beta = 0 (NaN-filled out), sub-view and res runs
    runs = lc.rs_runs(0, 8)
    assert {r[1] for r in runs} == set(lc.RS_LAYOUTS) and any(r[3] == 0.0 and r[1] == "subview" for r in runs)
    assert len({(a, b) for _, l, a, b in runs if l == "dense"}) == 9
    # babe_resample_res is legal somewhere for every mode
    for mode in range(4):
        assert any(lc.rs_res_legal(lc.rs_geometry("res", mode, 2, 3, 3, T)) for T in lc.RS_T)


def test_resample_inexact_restatement_stays_inside_the_bound():
    alpha = 1.0 / math.sqrt(2.0)
    for mode in range(4):
        for T in lc.RS_INEXACT_T:
            x, res = lc.rs_inputs(mode, (2, 3, 3), T, integers=False)
            ref = alpha * lc.resample64(mode, x, T) + res.double()
            if mode < 2:
                f32 = (UN.resample_down if mode == 0 else UN.resample_up)(x)
            else:
                z = torch.zeros(x.shape[:3] + (T,), requires_grad=True)
                f32, = torch.autograd.grad(((UN.resample_down if mode == 2 else UN.resample_up)(z) * x).sum(), z)
            got = torch.tensor(alpha, dtype=torch.float32) * f32 + res
            assert bool(((got.double() - ref).abs() <= lc.rs_inexact_bound(mode, x, res, T, alpha, 1.0)).all())


# ----------------------------------------------------------------------------- E. element-wise kernels
def test_axpby_table_reaches_what_it_names():
    seen = {}
    for name, B, C, Fq, T, inl, outl, V, _ in lc.AXPBY_CASES:
        assert lc.axpby_variant(B, C, Fq, T, inl, outl) == V, name
        seen[name] = lc.axpby_blocks(Fq * T, V)
        assert B * C * (Fq * T + max(inl[1], outl[1])) + 16 <= 1 << 20
    for name in ("big-vector", "big-scalar"):
        bx, sweep = seen[name]
        n = {"big-vector": 65540, "big-scalar": 16385}[name]
        assert bx == 64 and sweep < n < 2 * sweep                                         # a second turn, for the first threads only
    assert {c[0] for c in lc.AXPBY_CASES if c[7] == 1} == {"odd", "unaligned", "stride", "big-scalar"}
    for a, b in lc.AXPBY_EXACT:
        assert all(v == 0 or math.log2(abs(v)) % 1 == 0 for v in (a, b))
    # the one-pass merge: torch's float32 (a*x) + (b*y) rounds each product, then the sum - not an fma
    x, y = torch.tensor([1.0 + 2.0 ** -23]), torch.tensor([-(1.0 + 2.0 ** -22)])
    a = torch.tensor(1.0 + 2.0 ** -23)
    two_roundings = float((a * x) + (torch.tensor(1.0) * y))
    fused = float((a.double() * x.double() + y.double()).float())
    assert two_roundings != fused
    assert [Fq * T for Fq, T in lc.FILL_CASES] == [1, 1023, 65537]


@pytest.mark.parametrize("B,K,J", lc.LINEAR_CASES)
def test_linear_restatement_stays_inside_the_bound(B, K, J):
    x, W, bias = lc.linear_inputs(B, K, J)
    for b in (bias, None):
        for relu in (False, True):
            ref, bound = lc.linear_ref64(x, W, b, relu)
            got = x @ W.t() + (b if b is not None else 0)
            got = got.clamp_min(0) if relu else got
            assert bool(((got.double() - ref).abs() <= bound).all())
            want = torch.relu(UN.linear(x.double(), W.double(), b.double())) if relu and b is not None else None
            assert want is None or torch.equal(want, ref)
    assert -(-K // 64) == {1: 1, 63: 1, 65: 2}[K]
