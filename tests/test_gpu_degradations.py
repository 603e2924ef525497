"""predict_bwe's 'cheby1' / 'biquad' / 'resample' / 'decimate' degradations on the HIP kernels (csrc/degrade.hip,
csrc/resample_sinc.hip) against the reference's own operators and sampler (tests/golden/make_degradation_golden.py).
Needs a MI355X."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")


def load(name):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in np.load(os.path.join(G, name)).items()}


def rel_rows(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float(((a - b).norm(dim=-1) / (b.norm(dim=-1) + 1e-30)).max())


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def rms_err(a, b):
    return float((a.detach().double().cpu() - b.double().cpu()).pow(2).mean().sqrt())


def inputs(seed, L, scale=0.3):
    g = torch.Generator().manual_seed(int(seed))
    return scale * torch.randn(2, L, generator=g), torch.randn(2, L, generator=g)


def test_iir_forward_and_adjoint_vs_reference_fixture():
    from babe_amd.degrade import IIRDegradation
    d = {**load("degradation_ops_iir1k.npz"), **load("degradation_ops_iir3k.npz")}
    for i in sorted({int(k[5]) for k in d}):
        y_ref = d[f"cheby{i}_y"]
        x, w = inputs(d[f"cheby{i}_seed"], y_ref.shape[-1])
        A = IIRDegradation(d[f"cheby{i}_b"].numpy(), d[f"cheby{i}_a"].numpy(), clamp=False, device="cuda")
        assert rel_rows(A.fwd(x.cuda()), y_ref) <= 1e-5, i
        assert rel_rows(A.adj(w.cuda()), d[f"cheby{i}_gx"]) <= 1e-5, i


def test_biquad_resample_decimate_vs_reference_fixture():
    from babe_amd.degrade import DecimateDegradation, IIRDegradation, ResampleDegradation
    o = load("degradation_ops_other.npz")
    x, w = inputs(o["biquad_seed"], o["biquad_y"].shape[-1], scale=float(o["biquad_scale"]))
    c = o["biquad_coef"].numpy()
    A = IIRDegradation(c[:3], c[3:], clamp=True, device="cuda")
    y = A.fwd(x.cuda())
    assert (A.mask == 0).any()                                        # the clamp acts
    assert rel_rows(y, o["biquad_y"]) <= 1e-5 and rel_rows(A.adj(w.cuda()), o["biquad_gx"]) <= 1e-5
    L = o["resample0_gx"].shape[-1]
    for i in range(2):
        x, w = inputs(o[f"resample{i}_seed"], L)
        A = ResampleDegradation(float(o[f"resample{i}_factor"]), L)
        y = A.fwd(x.cuda())
        assert y.shape[-1] == o[f"resample{i}_y"].shape[-1] == A.out_length()
        assert rel_rows(y, o[f"resample{i}_y"]) <= 1e-5, i
        assert rel_rows(A.adj(w[:, :y.shape[-1]].contiguous().cuda()), o[f"resample{i}_gx"]) <= 1e-5, i
    L = o["decimate0_gx"].shape[-1]
    for i in range(2):
        x, w = inputs(o[f"decimate{i}_seed"], L)
        A = DecimateDegradation(int(o[f"decimate{i}_factor"]), L)
        y = A.fwd(x.cuda())
        assert torch.equal(y.cpu(), o[f"decimate{i}_y"])
        assert torch.equal(A.adj(w[:, :y.shape[-1]].contiguous().cuda()).cpu(), o[f"decimate{i}_gx"])


def _stable_den(order, radius=0.99):
    """Denominator with chosen poles of radius 0.99: conjugate pairs spread over the upper half plane, one real pole for odd
    orders (still stable once the coefficients are rounded to float32; a cheby1 of order 16 is not)."""
    n = order // 2
    th = (np.arange(n) + 0.5) * np.pi / max(n, 1)
    poles = list(radius * np.exp(1j * th)) + list(radius * np.exp(-1j * th))
    if order % 2:
        poles.append(radius)
    return np.real(np.poly(poles))


def _ref64(x, bn, an, adjoint=False):
    import scipy.signal
    xx = x.double().numpy()
    if adjoint:
        xx = xx[..., ::-1]
    y = scipy.signal.lfilter(bn.double().numpy(), an.double().numpy(), xx, axis=-1)
    return torch.from_numpy((y[..., ::-1] if adjoint else y).copy())


@pytest.mark.parametrize("order", [1, 2, 16])
def test_iir_chunk_edges_against_float64_recursion(order):
    from babe_amd.degrade import iir_filter, prepare_iir
    C = (order + 1) * (256 // (order + 1))                     # chunk length of csrc/degrade.hip
    rng = np.random.default_rng(order)
    b = rng.standard_normal(order + 1) * 0.1
    bn, an = prepare_iir(b, _stable_den(order))
    for L in (1, 7, C - 1, C, C + 1, 3 * C + 5, 368368):
        g = torch.Generator().manual_seed(L)
        x = torch.randn(2, L, generator=g)
        for adj in (False, True):
            y = iir_filter(x.cuda(), bn, an, adjoint=adj, prepared=True)
            assert rel_rows(y, _ref64(x, bn, an, adj)) <= 1e-5, (order, L, adj)


def test_adjoint_identity_for_all_four_types():
    from babe_amd.degrade import DecimateDegradation, IIRDegradation, ResampleDegradation
    from babe_amd.utils.bandwidth_extension import design_biquad_lpf, get_cheby1_ba
    L = 50001
    g = torch.Generator().manual_seed(5)
    x = (0.1 * torch.randn(2, L, generator=g)).cuda()
    c6 = design_biquad_lpf(3000, 22050, 0.707)
    ops = [IIRDegradation(*get_cheby1_ba(8, 0.05, 2 * 1000 / 22050), clamp=False, device="cuda"),
           IIRDegradation([float(v) for v in c6[:3]], [float(v) for v in c6[3:]], clamp=True, device="cuda"),
           ResampleDegradation(22050 / 2000, L), DecimateDegradation(5, L)]
    for A in ops:
        y = A.fwd(x)
        w = torch.randn(y.shape, generator=g).cuda()
        lhs = float((y.double() * w.double()).sum())
        rhs = float((x.double() * A.adj(w).double()).sum())
        assert abs(lhs - rhs) <= 1e-6 * (abs(lhs) + 1e-30) or abs(lhs - rhs) <= 1e-6 * float(y.double().norm() * w.double().norm()), \
            (type(A).__name__, lhs, rhs)


def test_iir_is_deterministic_and_rows_are_independent():
    from babe_amd.degrade import iir_filter, prepare_iir
    from babe_amd.utils.bandwidth_extension import get_cheby1_ba
    bn, an = prepare_iir(*get_cheby1_ba(8, 0.05, 2 * 3000 / 44100))
    g = torch.Generator().manual_seed(9)
    x = torch.randn(3, 368368, generator=g).cuda()
    for adj in (False, True):
        y1 = iir_filter(x, bn, an, adjoint=adj, prepared=True)
        y2 = iir_filter(x, bn, an, adjoint=adj, prepared=True)
        assert torch.equal(y1, y2)
        assert torch.equal(iir_filter(x[1:2], bn, an, adjoint=adj, prepared=True)[0], y1[1])


def test_biquad_clamp_mask():
    from babe_amd.degrade import iir_filter, prepare_iir
    from babe_amd.utils.bandwidth_extension import design_biquad_lpf
    c6 = design_biquad_lpf(3000, 22050, 0.707)
    bn, an = prepare_iir([float(v) for v in c6[:3]], [float(v) for v in c6[3:]])
    g = torch.Generator().manual_seed(3)
    x = (2.0 * torch.randn(2, 20000, generator=g)).cuda()
    free = iir_filter(x, bn, an, prepared=True)
    mask = torch.empty(x.shape, dtype=torch.uint8, device="cuda")
    y = iir_filter(x, bn, an, clamp=True, mask=mask, prepared=True)
    assert torch.equal(mask.bool(), free.abs() <= 1) and (mask == 0).any() and (mask == 1).any()
    assert torch.equal(y, free.clamp(-1, 1))
    w = torch.randn(x.shape, generator=g).cuda()
    assert torch.equal(iir_filter(w, bn, an, clamp=True, adjoint=True, mask=mask, prepared=True),
                       iir_filter(w * mask.float(), bn, an, adjoint=True, prepared=True))
    with pytest.raises(ValueError):
        iir_filter(w, bn, an, clamp=True, adjoint=True, prepared=True)


def _sampler(start_sigma, dc=False):
    from babe_amd.diff_params.edm import EDM
    from babe_amd.testing.blind_bwe_sampler import BlindSampler
    from tests.test_gpu_sampler import ResidualNet, small_net
    g, args, net = small_net(T=3, start_sigma=start_sigma)
    args.tester.posterior_sampling.data_consistency = dc
    return BlindSampler(ResidualNet(net, 0.3, 0.063), EDM(args), args)


def _feed(smp, seed, L=92092):
    gen = torch.Generator().manual_seed(int(seed))
    it = iter([torch.randn(1, L, generator=gen) for _ in range(4)])
    smp._randn = lambda shape, device: next(it).to(device)


@pytest.mark.parametrize("name", ["cheby1", "cheby1_dc", "biquad"])
def test_predict_bwe_iir_vs_reference_golden(name):
    from babe_amd.utils.bandwidth_extension import design_biquad_lpf, get_cheby1_ba
    ftype = name.split("_")[0]
    s = load(f"degradation_sampler_{ftype}.npz")
    smp = _sampler(0.05, dc=name.endswith("_dc"))
    _feed(smp, s[f"{name}_seed"])
    filt = get_cheby1_ba(6, 0.05, 2 * 3000 / 22050) if ftype == "cheby1" else design_biquad_lpf(3000, 22050, 0.707)
    x, dden, dscore, t = smp.predict_bwe(s[f"{ftype}_y"].cuda(), filt, ftype, rid=True)
    assert torch.equal(t, s[f"{name}_t"])
    for i in range(3):
        assert rel(dden[i][:, ::16], s[f"{name}_den_sub16"][i]) < 1e-3, i
        if i < 2:
            assert rel(dscore[i][:, ::16], s[f"{name}_score_sub16"][i]) < 2e-3, i
    xs = x[:, ::4]
    assert rms_err(xs, s[f"{name}_x_sub4"]) < 1e-3 and rel(xs, s[f"{name}_x_sub4"]) < 2e-3
    assert smp.degradation is None


@pytest.mark.parametrize("ftype,filt", [("resample", 22050 / 4000), ("decimate", 2)])
def test_predict_bwe_resample_decimate_vs_reference_golden(ftype, filt):
    s = load("degradation_sampler_rs.npz")
    smp = _sampler("None")
    _feed(smp, s[f"{ftype}_seed"])
    x = smp.predict_bwe(s[f"{ftype}_y"].cuda(), filt, ftype, rid=True)       # x alone, whatever rid is (:376-385)
    assert torch.is_tensor(x) and x.shape == (1, 92092)
    xs = x[:, ::4]
    assert rms_err(xs, s[f"{ftype}_x_sub4"]) < 1e-3 and rel(xs, s[f"{ftype}_x_sub4"]) < 2e-3


def test_library_evaluation_falls_back_for_the_new_degradations():
    from babe_amd.degrade import (DecimateDegradation, FIRDegradation, IIRDegradation, MaskDegradation, MaskMixDegradation,
                                  ResampleDegradation)
    from babe_amd.testing import eval_c
    smp = _sampler(0.05)
    y = torch.zeros(1, 92092, device="cuda")
    fir, mask = FIRDegradation(torch.ones(5) / 5, "cuda"), torch.ones(1, 92092, device="cuda")
    for deg in (IIRDegradation([0.5, 0.5], [1.0, -0.5], clamp=False, device="cuda"), DecimateDegradation(2, 92092),
                ResampleDegradation(2.0, 92092), fir, MaskDegradation(mask, "cuda"), MaskMixDegradation(mask, fir),
                MaskMixDegradation(mask, None)):
        smp.degradation = deg
        assert not eval_c.supported(smp, y, False), type(deg).__name__
        assert not smp._use_lanes(2, y, False, torch.zeros(2, 2, 1)), type(deg).__name__
