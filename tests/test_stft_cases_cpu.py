"""The float64 references and the case tables of tests/test_gpu_stft_edges.py, pinned without a GPU: the transforms against
torch.stft and the oracle, one step of the fit against the oracle's float32 fit_params and against finite differences, and every
row of every table reaching what its comment says."""
import numpy as np
import pytest
import torch

from oracle import bwe_utils as U
from tests import stft_cases as sc

SMALL = [c for c in sc.TRANSFORM_CASES if c[0] <= 1024]


@pytest.mark.parametrize("c", SMALL, ids=[sc.transform_id(c) for c in SMALL])
def test_stft64_is_torch_stft_of_the_zero_extended_signal(c):
    nfft, L = c[:2]
    x = sc.transform_inputs(nfft, L)[0].double()
    xp = torch.cat((x, torch.zeros(x.shape[0], nfft, dtype=torch.float64)), 1)
    ref = torch.stft(xp, nfft, hop_length=nfft // 2, window=torch.hamming_window(nfft, dtype=torch.float64), center=False,
                     return_complex=True).transpose(1, 2)
    got = sc.stft64(x, nfft)
    assert got.shape == ref.shape == (x.shape[0], sc.n_frames(L, nfft), nfft // 2 + 1)
    assert float((got - ref).abs().max() / ref.abs().max()) < 1e-13
    assert torch.equal(sc.frames64(x, nfft)[:, -1, max(0, L - (got.shape[1] - 1) * (nfft // 2)):],
                       torch.zeros(x.shape[0], nfft - max(0, L - (got.shape[1] - 1) * (nfft // 2)), dtype=torch.float64))


@pytest.mark.parametrize("c", SMALL, ids=[sc.transform_id(c) for c in SMALL])
def test_analysis_synthesis_is_the_identity_and_the_oracles_apply_filter(c):
    nfft, L = c[:2]
    x, _, _, H = sc.transform_inputs(nfft, L)
    T = sc.n_frames(L, nfft)
    env = sc.env_inv64(nfft, T)
    rec = sc.ola64(sc.filtered_frames64(sc.stft64(x, nfft), 1.0, nfft), L, env)
    assert float((rec - x.double()).abs().max() / x.abs().max()) < 1e-13
    assert float((rec - U.apply_filter(x.double(), torch.ones(nfft // 2 + 1, dtype=torch.float64), nfft)).abs().max()) < 1e-13
    filt = sc.ola64(sc.filtered_frames64(sc.stft64(x, nfft), H[0].double(), nfft), L, env)
    ref = U.apply_filter(x.double(), H[0].double(), nfft)
    assert float((filt - ref).abs().max() / ref.abs().max()) < 1e-13
    # residual mode, and a filter per clip
    r, ss = sc.ola64(sc.filtered_frames64(sc.stft64(x, nfft), H.double(), nfft), L, env, y=x)
    for b in range(x.shape[0]):
        rb = x[b].double() - U.apply_filter(x[b:b + 1].double(), H[b].double(), nfft)[0]
        assert float((r[b] - rb).abs().max()) < 1e-13 and abs(float(ss[b]) - float((rb * rb).sum())) < 1e-12 * float(ss[b])


def test_filtered_frames64_ignores_the_imaginary_parts_at_dc_and_nyquist():
    nfft, L = 256, 389
    spec = sc.as_complex(sc.transform_inputs(nfft, L)[2])
    assert float(spec[..., 0].imag.abs().min()) > 0 and float(spec[..., -1].imag.abs().min()) > 0
    real_ends = spec.clone()
    real_ends[..., 0] = real_ends[..., 0].real.to(torch.complex128)
    real_ends[..., -1] = real_ends[..., -1].real.to(torch.complex128)
    assert torch.equal(sc.filtered_frames64(spec, 1.0, nfft), sc.filtered_frames64(real_ends, 1.0, nfft))
    # against the explicit inverse sum, one frame
    n = torch.arange(nfft, dtype=torch.float64)
    k = torch.arange(1, nfft // 2, dtype=torch.float64)
    z = real_ends[0, 0]
    ang = 2 * np.pi * k[:, None] * n[None, :] / nfft
    direct = (z[0].real + z[-1].real * (-1.0) ** n + 2 * (z[1:-1].real[:, None] * torch.cos(ang) - z[1:-1].imag[:, None] * torch.sin(ang)).sum(0)) / nfft
    got = sc.filtered_frames64(spec, 1.0, nfft)[0, 0]
    assert float((got - direct * sc.window64(nfft)).abs().max()) < 1e-12


def test_stats64_shared_is_the_sum_over_the_batch():
    X, Y = (sc.as_complex(sc.transform_inputs(256, 1000, B=3, seed=s)[2]) for s in (1, 2))
    per, sh = sc.stats64(X, Y, False), sc.stats64(X, Y, True)
    assert per.shape == (3, 3, 129) and sh.shape == (1, 3, 129)
    assert float((per.sum(0) - sh[0]).abs().max()) < 1e-12 * float(sh.max())
    assert float((per[1, 1] - (X[1].abs() * Y[1].abs()).sum(0)).abs().max()) == 0.0


def test_framed_err_sees_one_bad_frame_and_insists_on_exact_zeros():
    ref = sc.frames64(sc.transform_inputs(256, 128)[0], 256)                 # second frame all zero
    assert bool((ref[:, 1] == 0).all()) and sc.framed_err(ref.clone(), ref) == 0.0
    bad = ref.clone()
    bad[1, 0, 17] += 2 * sc.BAR * ref[1, 0].abs().max()
    assert sc.framed_err(bad, ref) > sc.BAR
    bad = ref.clone()
    bad[0, 1, 3] = 1e-30
    with pytest.raises(AssertionError):
        sc.framed_err(bad, ref)
    spec = sc.stft64(sc.transform_inputs(256, 128)[0], 256)[:, :1]            # no zero anywhere: an unwritten result is NaN
    assert np.isnan(sc.framed_err(torch.full_like(spec, float("nan")), spec))


def test_transform_table_is_well_formed():
    ids = [sc.transform_id(c) for c in sc.TRANSFORM_CASES]
    assert len(set(ids)) == len(ids)
    assert {c[0] for c in sc.TRANSFORM_CASES} == {256, 512, 1024, 2048, 4096}
    for nfft in (256, 512, 1024, 2048, 4096):
        assert (nfft, 3 * (nfft // 2) + 5, ) in [c[:2] for c in sc.TRANSFORM_CASES]
    frames = {c[1]: sc.n_frames(c[1], 256) for c in sc.TRANSFORM_CASES if c[0] == 256}
    assert frames == {389: 4, 100: 1, 128: 2, 129: 2, 383: 3, 1000: 8}
    assert max(c[1] for c in sc.TRANSFORM_CASES) == 3 * 2048 + 5                 # nothing longer is needed
    for nfft, L, _ in sc.TRANSFORM_CASES:
        x = sc.transform_inputs(nfft, L)[0]
        assert sc.frames64(x, nfft).shape == (sc.B_TRANSFORM, sc.n_frames(L, nfft), nfft)
        assert sc.env_inv64(nfft, sc.n_frames(L, nfft)).numel() >= L


# ----------------------------------------------------------------------------- the fit
def test_fit_table_is_well_formed():
    names = [c["name"] for c in sc.FIT_CASES]
    assert len(set(names)) == len(names)
    assert [f"K{K}-nfft4096" in names for K in range(1, 9)] == [True] * 8
    for c in sc.FIT_CASES:
        stats, params, f, cfg = sc.fit_inputs(c)
        P = params.shape[0]
        assert stats.shape == (P, 3, c["nfft"] // 2 + 1) and params.shape == (P, 2, c["K"]) and stats.dtype == torch.float64
        assert bool((stats > 0).all()) and 1 <= c["K"] <= 8
        df = c["fs"] / c["nfft"]
        for p in range(P):
            fc = params[p, 0]
            assert bool((fc[1:] > fc[:-1]).all()), f"{c['name']}: fc is not sorted"          # the anchor chain j -> j + 1
            assert bool((fc <= c["fs"] / 2).all()) and bool((fc > 0).all())
            on = [bool((f == v).any()) for v in fc]
            assert any(on) == c["on_bin"], f"{c['name']}: fc on a bin frequency: {on}"
        if c["name"] == "on-bin":
            assert df == 8.0 and bool((f == 8.0 * torch.arange(2049)).all()) and all(on)
    assert sc.FIT_BY_NAME["P3"]["params"] is not None and len(sc.FIT_BY_NAME["P3"]["params"]) == 3
    assert {c["cfg"].get("weighting", "sqrt") for c in sc.FIT_CASES} == {"None", "sqrt", "linear", "log"}


def _step(name, **over):
    c = sc.FIT_BY_NAME[name]
    stats, params, f, cfg = sc.fit_inputs(c)
    return params[0].double(), sc.fit_step64(stats[0], params[0], f, {**cfg, **over}), cfg


def test_fit_flag_rows_reach_the_branch_they_name():
    # each switch changes the result of its row
    for name, flag in (("no-clamp_fc", "clamp_fc"), ("no-clamp_A", "clamp_A")):
        _, (_, _, off), _ = _step(name)
        _, (_, _, on), _ = _step(name, **{flag: True})
        assert not torch.equal(off, on), name
    p, (_, _, q), cfg = _step("positive-A")
    assert q[1, 0] == cfg["Amax"] and bool((q[1, 1:] > 0).all()) and bool((q[1, 1:] < cfg["Amax"]).all()), q[1]
    _, (_, _, qneg), _ = _step("positive-A", only_negative_A=True)
    assert bool((qneg[1] <= -1.0).all())
    p, (_, g, q), cfg = _step("every-clamp")
    raw = p - torch.tensor(cfg["mu"], dtype=torch.float64)[:, None] * g
    assert q[0, 0] == cfg["fcmin"] > raw[0, 0] and q[0, 1] == q[0, 0] + 1 > raw[0, 1] and q[0, 3] == cfg["fcmax"] < raw[0, 3]
    assert q[0, 2] == raw[0, 2]
    assert q[1, 0] == raw[1, 0] and q[1, 1] == q[1, 0] < raw[1, 1] and q[1, 3] == cfg["Amin"] > raw[1, 3]
    # the three edge parameter sets: finite, and where the comment says
    f = U.bin_freqs(4096, sc.FS)
    fcs = torch.tensor(sc.FIT_BY_NAME["same-bin"]["params"][0][0])
    assert len({int(torch.nonzero(f >= v)[0, 0]) for v in fcs}) == 1 and float(fcs[-1] - fcs[0]) == 2.0
    assert float(f[-1]) == 22050.0 == sc.FIT_BY_NAME["nyquist"]["params"][0][0][-1]
    assert sc.FIT_BY_NAME["below-bin-1"]["params"][0][0][0] < float(f[1])
    for name in ("same-bin", "nyquist", "below-bin-1", "on-bin"):
        _, (loss, g, q), _ = _step(name)
        assert np.isfinite(loss) and bool(torch.isfinite(g).all()) and bool(torch.isfinite(q).all()) and bool((g[0] != 0).all()), name
    assert _step("below-bin-1")[1][2][0, 0] == 20.0


@pytest.mark.parametrize("K,nfft", [(1, 1024), (3, 1024), (5, 256)])
def test_fit_step64_vs_the_oracles_float32_fit_params(K, nfft):
    """Statistics of real magnitudes (the oracle's own float32 STFT), one iteration.  The oracle differentiates in float32 with
    its default flags; its gradient is within 1e-6 of float64 relative to the row's maximum, so the step agrees within
    step_bounds at 1e-5 (ten times that, plus 2 ulp of the parameter)."""
    g = torch.Generator().manual_seed(5 * K + nfft)
    L = 12 * nfft
    x = 0.1 * torch.randn(2, L, generator=g)
    f = U.bin_freqs(nfft, sc.FS)
    y = U.apply_filter(x, U.design_filter(torch.tensor([2500.0]), torch.tensor([-25.0]), f), nfft) + 1e-3 * torch.randn(2, L, generator=g)
    p0 = sc.random_params(K, 900 + K)
    mu = (100.0, 1.0)
    pref, nit = U.fit_params(x, y, p0, sc.FS, nfft=nfft, mu=mu, max_iter=1)
    Xm, Ym = U.stft(x, nfft).abs().double(), U.stft(y, nfft).abs().double()        # [B, bins, frames]
    stats = torch.stack([(Xm * Xm).sum((0, 2)), (Xm * Ym).sum((0, 2)), (Ym * Ym).sum((0, 2))])
    loss, grad, q = sc.fit_step64(stats, p0, f, dict(mu=mu, fcmax=sc.FS // 2))
    assert nit == 1
    lref = float(U.mag_loss(Xm.float(), Ym.float(), U.design_filter(p0[0], p0[1], f), U.freq_weight(f.numel(), "sqrt")))
    assert abs(loss - lref) < 2e-6 * lref
    assert bool(((pref.double() - q).abs() <= sc.step_bounds(grad, q, mu, 1e-5)).all()), (pref, q)
    assert not torch.equal(q, p0.double())


def test_fit_step64_gradient_vs_central_differences():
    """K = 3 with the breakpoints away from bin frequencies (a mask must not flip inside the difference)."""
    f = U.bin_freqs(4096, sc.FS)
    p = torch.tensor([[1234.5, 3456.7, 8901.2], [-7.0, -13.0, -21.0]])
    assert float((f[None, :] - p[0][:, None]).abs().min()) > 0.5
    stats = sc.synth_stats(f, 5)
    _, grad, _ = sc.fit_step64(stats, p, f, {})
    pd = p.double()
    for i in range(2):
        for j in range(3):
            h = 1e-3 if i == 0 else 1e-6
            up, dn = pd.clone(), pd.clone()
            up[i, j] += h
            dn[i, j] -= h
            fd = (float(sc.fit_objective64(stats, up, f.double(), "sqrt")) - float(sc.fit_objective64(stats, dn, f.double(), "sqrt"))) / (2 * h)
            assert abs(fd - float(grad[i, j])) < 1e-6 * float(grad[i].abs().max()), (i, j, fd, float(grad[i, j]))


def test_gradient_read_off_case_resolves_its_bar():
    """4b: with mu = (1, 1) and no clamp the step IS the gradient, stored as a float32 difference from the parameter; the statistics
    are scaled so that half a float32 spacing of fc is below a tenth of the 5e-4 ceiling on every row."""
    for K in sc.GRAD_KS:
        stats, params, f, cfg = sc.grad_inputs(K)
        _, g, q = sc.fit_step64(stats[0], params[0], f, cfg)
        assert torch.equal(q, params[0].double() - g)
        for i in range(2):
            half_ulp = 0.5 * float(torch.maximum(sc.ulp32(q[i]), sc.ulp32(params[0, i].double())).max())
            assert half_ulp < 5e-5 * float(g[i].abs().max()), (K, i, half_ulp, float(g[i].abs().max()))


def test_exact_statistics_bound_every_step_below_the_tolerance():
    stats, params, f, cfg = sc.exact_inputs()
    loss, g, _ = sc.fit_step64(stats[0], params[0], f, cfg)
    assert loss < 1e-9 * float(stats[0, 0].sum().sqrt())                         # Y = X H(p*): no residual in float64
    # any unit residual direction r: |J^T r| <= column norms, and mu times those is tol / 8
    w = U.freq_weight(f.numel(), "sqrt").double()
    J = torch.autograd.functional.jacobian(lambda q: w * torch.sqrt(stats[0, 0]) * U.design_filter(q[0], q[1], f.double()), params[0].double())
    worst = J.reshape(f.numel(), 2, 3).norm(dim=0) * torch.tensor(cfg["mu"], dtype=torch.float64)[:, None]
    assert float(worst.max()) <= 5e-3 / 8 * (1 + 1e-9)


@pytest.mark.parametrize("name", list(sc.DESIGN_CASES))
def test_design_rows(name):
    fc, A = (torch.tensor(v) for v in sc.DESIGN_CASES[name])
    assert bool((fc[1:] > fc[:-1]).all()) == (not name.startswith("unsorted"))
    for nfft in (256, 4096):
        f = U.bin_freqs(nfft, sc.FS)
        H64 = U.design_filter(fc.double(), A.double(), f.double())
        H32 = U.design_filter(fc, A, f)
        assert bool(torch.isfinite(H64).all()) and torch.equal(H64 == 1.0, H32 == 1.0)
        assert float(((H32.double() - H64).abs() / H64).max()) < 3e-6
