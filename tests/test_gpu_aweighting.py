"""A-weighted training loss on the GPU: the fused kernels babe_fir_sqerr_fwd / _bwd (csrc/loss.hip) against float64 F.conv1d and
its autograd on the CPU, the adjoint identity, run-to-run and stream independence, the refusals, FIRFilter and EDM.loss_fn against
the reference's own outputs (tests/golden/aweighting.npz, make_aweighting_golden.py) and one SGD step of the reduced-width
network under the weighted loss.  Needs a MI355X."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
OP_BAR = 3e-6                          # README: ops <= 3e-6 of the largest reference value
TILE = 2048                            # outputs per workgroup of fir_sqerr_kernel (LS_TILE); its two runs per thread meet at 1024
LENGTHS = (1, 37, 100, 101, 257, 4099, TILE - 1, TILE, TILE + 1)
TAPS = (1, 3, 101, 255)
B = 2


def fixture():
    return np.load(os.path.join(G, "aweighting.npz"))


@functools.lru_cache(maxsize=None)
def case(L, K):
    """Seeded operands (est and g as views with row stride L + 3) and the float64 CPU reference, computed once per shape."""
    gen = torch.Generator().manual_seed(1000 * K + L)
    est = torch.randn(B, L + 3, generator=gen)[:, :L]
    tgt = torch.randn(B, L, generator=gen)
    taps = torch.randn(K, generator=gen)                               # asymmetric
    g = torch.randn(B, L + 3, generator=gen)[:, :L]
    d = (est - tgt).double().requires_grad_(True)                      # the float32 difference, as the kernel forms it
    ew = F.conv1d(d[:, None], taps.double()[None, None], padding=K // 2)[:, 0]
    err2 = ew ** 2
    grad, = torch.autograd.grad((g.double() * err2).sum(), d)          # d err2 / d est = d err2 / d d
    return dict(est=est, tgt=tgt, taps=taps, g=g, ew=ew.detach(), err2=err2.detach(), grad=grad)


def strided_cuda(t):
    """The same values on the device with the same row stride (L + 3)."""
    Bq, L = t.shape
    buf = torch.full((Bq, L + 3), float("nan"), device="cuda")
    buf[:, :L] = t.cuda()
    v = buf[:, :L]
    assert v.stride() == (L + 3, 1)
    return v


def relmax(got, want):
    return float((got.double().cpu() - want).abs().max() / want.abs().max())


@pytest.mark.parametrize("K", TAPS)
def test_forward_vs_float64_conv1d(K):
    from babe_amd.stft import fir_sqerr
    worst = 0.0
    for L in LENGTHS:
        c = case(L, K)
        err2, ew = fir_sqerr(strided_cuda(c["est"]), c["tgt"].cuda(), c["taps"].cuda(), return_filtered=True)
        assert err2.shape == ew.shape == (B, L) and err2.is_contiguous() and ew.is_contiguous()
        e_ew, e_err2 = relmax(ew, c["ew"]), relmax(err2, c["err2"])
        print(f"K {K} L {L}: ew {e_ew:.2e} err2 {e_err2:.2e}")
        worst = max(worst, e_ew, e_err2)
        assert e_ew <= OP_BAR and e_err2 <= OP_BAR, (K, L, e_ew, e_err2)
        assert torch.equal(err2, ew * ew)
    print(f"K {K}: worst {worst:.2e}")


@pytest.mark.parametrize("K", TAPS)
def test_backward_vs_float64_autograd(K):
    from babe_amd.stft import fir_sqerr
    for L in LENGTHS:
        c = case(L, K)
        est = strided_cuda(c["est"]).requires_grad_(True)
        tgt, taps = c["tgt"].cuda().requires_grad_(True), c["taps"].cuda().requires_grad_(True)
        err2 = fir_sqerr(est, tgt, taps)
        got, g_tgt, g_taps = torch.autograd.grad(err2, [est, tgt, taps], grad_outputs=strided_cuda(c["g"]), allow_unused=True)
        assert g_tgt is None and g_taps is None                        # the gradient with respect to est only
        e = relmax(got, c["grad"])
        print(f"K {K} L {L}: grad {e:.2e}")
        assert got.shape == (B, L) and e <= OP_BAR, (K, L, e)


def _fir_T(h, taps):
    """FIR^T h through babe_fir_sqerr_bwd: it filters 2 * g * ew, which is h exactly for g = 1/2, ew = h."""
    from babe_amd._lib import check, lib, ptr, stream
    half = torch.full_like(h, 0.5)
    out = torch.empty_like(h)
    check(lib().babe_fir_sqerr_bwd(ptr(half), half.stride(0), ptr(h), ptr(taps), taps.numel(), ptr(out), h.shape[0], h.shape[1],
                                   stream()), "fir_sqerr_bwd")
    return out


@pytest.mark.parametrize("K", TAPS)
def test_adjoint_identity(K):
    """<FIR e, h> = <e, FIR^T h>, both sums in float64 on the host.  h = FIR e / 2 + noise, so that the inner product is of the
    size of |FIR e| |h| and 1e-5 of it is a meaningful bound."""
    from babe_amd.stft import fir_sqerr
    for L in LENGTHS:
        c = case(L, K)
        e, taps = c["est"].contiguous(), c["taps"].cuda()
        gen = torch.Generator().manual_seed(L + K)
        _, fe = fir_sqerr(e.cuda(), torch.zeros(B, L, device="cuda"), taps, return_filtered=True)        # FIR e
        h = (0.5 * fe.cpu() + torch.randn(B, L, generator=gen)).contiguous()
        lhs = float((fe.double().cpu() * h.double()).sum())
        rhs = float((e.double() * _fir_T(h.cuda(), taps).double().cpu()).sum())
        print(f"K {K} L {L}: <FIR e, h> {lhs:.9g}  <e, FIR^T h> {rhs:.9g}")
        assert abs(lhs - rhs) <= 1e-5 * abs(lhs), (K, L, lhs, rhs)


def test_deterministic_and_stream_independent():
    from babe_amd.stft import fir_sqerr
    c = case(4099, 101)
    est, tgt, taps, g = strided_cuda(c["est"]), c["tgt"].cuda(), c["taps"].cuda(), c["g"].cuda()

    def run():
        x = est.detach().requires_grad_(True)
        err2, ew = fir_sqerr(x, tgt, taps, return_filtered=True)
        gx, = torch.autograd.grad(err2, x, grad_outputs=g)
        return err2.detach(), ew, gx

    a, b = run(), run()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s = run()
    side.synchronize()
    for x, y, z in zip(a, b, s):
        assert torch.equal(x, y) and torch.equal(x, z)


@pytest.mark.parametrize("K", [0, 2, 100, 257])
def test_invalid_tap_count_is_refused_with_nothing_written(K):
    from babe_amd._lib import BabeHipError, lib, ptr, stream
    from babe_amd.stft import fir_sqerr
    L = 300
    est, tgt, taps = torch.randn(B, L, device="cuda"), torch.randn(B, L, device="cuda"), torch.randn(max(K, 1), device="cuda")
    ew, err2, dest = (torch.full((B, L), -7.0, device="cuda") for _ in range(3))
    assert lib().babe_fir_sqerr_fwd(ptr(est), L, ptr(tgt), L, ptr(taps), K, ptr(ew), ptr(err2), B, L, stream()) != 0
    assert lib().babe_fir_sqerr_bwd(ptr(est), L, ptr(tgt), ptr(taps), K, ptr(dest), B, L, stream()) != 0
    torch.cuda.synchronize()
    assert bool((ew == -7.0).all()) and bool((err2 == -7.0).all()) and bool((dest == -7.0).all())
    if K > 0:
        with pytest.raises(BabeHipError):
            fir_sqerr(est, tgt, taps)


@pytest.mark.parametrize("ft", ["hp", "fd"])
def test_firfilter_asymmetric_vs_reference_fixture(ft):
    """The reference's FIRFilter("hp") / ("fd") on a [2, 37] tensor: a kernel that flipped the taps would fail here (the
    A-weighting taps are symmetric).  The backward is the transposed FIR: against float64 autograd of F.conv1d."""
    from babe_amd.utils.training_utils import FIRFilter
    f = fixture()
    e = torch.from_numpy(f["asym_in"])
    want = torch.from_numpy(f["asym_" + ft]).double()
    filt = FIRFilter(ft)
    x = e.cuda().requires_grad_(True)
    y = filt(x)
    assert filt.taps.is_cuda and relmax(y, want) <= OP_BAR
    w = torch.randn(e.shape, generator=torch.Generator().manual_seed(2))
    gx, = torch.autograd.grad(y, x, grad_outputs=w.cuda())
    e64 = e.double().requires_grad_(True)
    y64 = F.conv1d(e64[:, None], torch.from_numpy(f["taps_" + ft]).double()[None, None], padding=1)[:, 0]
    g64, = torch.autograd.grad(y64, e64, grad_outputs=w.double())
    assert relmax(gx, g64) <= OP_BAR


def fixture_edm(f, aweighting):
    from babe_amd.config import default_args, to_attr
    from babe_amd.diff_params.edm import EDM
    args = default_args(sample_rate=int(f["loss_fs"]))
    dp = args.diff_params
    dp.sigma_min, dp.sigma_max, dp.ro_train, dp.sigma_data = (float(v) for v in f["dp"])
    dp.aweighting = to_attr(dict(use_aweighting=aweighting, ntaps=int(f["loss_ntaps"])))
    return EDM(args)


@pytest.mark.parametrize("tag", ["long", "short"])
def test_loss_fn_vs_reference_fixture(tag, monkeypatch):
    """EDM.loss_fn with A-weighting against the reference's (L = 400, and L = 50 < 101 taps), on the recorded draws."""
    f = fixture()
    t = lambda k: torch.from_numpy(np.asarray(f[f"{tag}_{k}"]))
    edm = fixture_edm(f, True)
    a, b = (float(v) for v in f["stub"])
    x = t("x")
    torch.manual_seed(int(f["loss_seed"]))
    u, z = torch.rand(x.shape[0]), torch.randn(x.shape)               # the recorded draws: sigma's uniform, then the noise
    assert torch.allclose(z * t("sigma"), t("noise"), rtol=1e-6, atol=1e-7)
    monkeypatch.setattr(torch, "rand", lambda *s, **k: u.clone())
    monkeypatch.setattr(torch, "randn", lambda *s, **k: z.clone())
    seen = {}

    def stub(inp, cnoise):
        seen["input"], seen["cnoise"] = inp, cnoise
        return a * inp + b * cnoise

    err2, sigma = edm.loss_fn(stub, x.cuda())
    monkeypatch.undo()
    assert torch.equal(sigma.cpu(), t("sigma"))
    assert torch.allclose(seen["input"].cpu(), t("input"), rtol=1e-6, atol=1e-7)
    assert torch.allclose(seen["cnoise"].cpu(), t("cnoise"), rtol=1e-6, atol=1e-7)
    e = relmax(err2, t("err2").double())
    print(f"{tag}: err2 vs the reference {e:.2e}")
    assert err2.shape == x.shape and e <= OP_BAR


def test_aweighting_off_is_the_two_torch_ops():
    f = fixture()
    edm = fixture_edm(f, False)
    x = torch.from_numpy(f["long_x"]).cuda()
    stub = lambda inp, cnoise: 0.5 * inp - 0.25 * cnoise
    torch.manual_seed(9)
    err2, sigma = edm.loss_fn(stub, x)
    torch.manual_seed(9)
    s = edm.sample_ptrain_safe(x.shape[0]).unsqueeze(-1).to(x.device)
    inp, target, cnoise = edm.prepare_train_preconditioning(x, s)
    assert torch.equal(sigma, s) and torch.equal(err2, (stub(inp, cnoise) - target) ** 2)


def test_sgd_step_lowers_aweighted_loss_first_order():
    """The recipe of tests/test_gpu_unet_train.py::test_sgd_step_lowers_loss_first_order under the A-weighted loss: fir_sqerr's
    backward feeds the network's parameter-gradient path."""
    from babe_amd.config import default_args, to_attr
    from babe_amd.diff_params.edm import EDM
    from babe_amd.networks.cqtdiff_plus import Unet_CQT_oct_with_attention
    L, Ns = 92092, [8, 8, 8, 8, 16, 16, 16]
    args = default_args(sample_rate=22050, audio_len=L, Ns=Ns)
    args.diff_params.aweighting = to_attr(dict(use_aweighting=True, ntaps=101))
    edm = EDM(args)
    u = {k: torch.from_numpy(np.asarray(v)) for k, v in np.load(os.path.join(G, "unet_small.npz")).items()}
    net = Unet_CQT_oct_with_attention(args, "cuda")
    net.load_state_dict({k[3:]: v for k, v in u.items() if k.startswith("sd.")}, strict=True)
    net.set_trainable(True)
    x = (0.1 * torch.randn(2, L, generator=torch.Generator().manual_seed(5))).cuda()

    def loss():
        torch.manual_seed(7)
        return edm.loss_fn(net, x)[0].mean()

    l0 = loss()
    l0.backward()
    gn2 = sum(float((p.grad.double() ** 2).sum()) for p in net.parameters() if p.grad is not None)
    lr = 1e-3 / gn2 ** 0.5 * float(l0.detach())
    with torch.no_grad():
        for p in net.parameters():
            if p.grad is not None:
                p -= lr * p.grad
        l1 = loss()
    want = lr * gn2
    print(f"loss {float(l0):.6g} -> {float(l1):.6g}: decrease {float(l0 - l1):.4g}, predicted {want:.4g}")
    assert float(l0 - l1) > 0 and abs(float(l0 - l1) - want) < 0.2 * want
