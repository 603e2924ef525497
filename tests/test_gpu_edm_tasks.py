"""Declipping, compressed sensing and phase retrieval on the GPU: the clip and STFT-magnitude operators against float64 torch on
the CPU (torch.clip / torch.stft with autograd), and the three sampler entry points against the reference's own runs
(tests/golden/edm_sampler_tasks.npz, written by tests/golden/make_edm_tasks_golden.py).  Needs a MI355X."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
TOL = 1e-5                 # relative, per row: the bar of the degradation operators


def load(name):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in np.load(os.path.join(G, name)).items()}


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def rms_err(a, b):
    return float((a.detach().double().cpu() - b.double().cpu()).pow(2).mean().sqrt())


def row_rel(a, b):
    a, b = a.detach().double().cpu().reshape(a.shape[0], -1), b.detach().double().cpu().reshape(b.shape[0], -1)
    return float(((a - b).norm(dim=1) / b.norm(dim=1).clamp_min(1e-300)).max())


# ---- clip -----------------------------------------------------------------------------------------------------------------
def _clip_case(L):
    c = 0.5
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, L, generator=g)
    x[1] = 0.4 * torch.rand(L, generator=g) - 0.2            # a row with no sample above c
    x[0, 3], x[0, 4], x[0, L - 1], x[1, 7] = c, -c, c, -c         # samples exactly at the bounds: inside the closed interval
    x[0, 5], x[0, 6] = float(np.nextafter(np.float32(c), np.float32(1))), -float(np.nextafter(np.float32(c), np.float32(1)))
    y = torch.randn(2, L, generator=g)
    gs = torch.randn(2, L, generator=g)
    return c, x, y, gs, x.cuda(), y.cuda(), gs.cuda()


@pytest.mark.parametrize("L", [1003, 1004, 70000, 9])
def test_clip_forward_residual_mask_and_adjoint_are_exact(L):
    """1003 with B = 2: the second row is not 16-byte aligned, the element-wise path; its first row alone (B = 1): the 16-byte
    path with a ragged last vector; 1004: the 16-byte path, a part-filled chunk; 70000: more than one pass of the 64 blocks
    (64 x 4 x 256 = 65536 samples per pass); 9: shorter than a chunk."""
    from babe_amd.degrade import ClipDegradation, clip_residual, sumsq_partial
    c, x, y, gs, xd, yd, gd = _clip_case(L)
    deg = ClipDegradation(c)
    want = torch.clip(x, -c, c)
    mask_want = (x.abs() <= c)
    assert bool(mask_want[1].all()) and not bool(mask_want[0].all())
    assert torch.equal(deg.fwd(xd).cpu(), want)
    r, mask, part = clip_residual(xd, yd, c)
    assert torch.equal(r.cpu(), y - want)
    assert mask.dtype == torch.uint8 and torch.equal(mask.cpu().bool(), mask_want)
    assert part.shape == (2, 64) and torch.equal(part, sumsq_partial(r))
    r2, part2 = deg.residual(xd, yd)
    assert torch.equal(r2, r) and torch.equal(part2, part)
    got = deg.adj(gd)
    assert torch.equal(got.cpu(), gs * mask_want)
    xa = x.clone().requires_grad_(True)                      # torch's own gradient of clip is that mask
    ga, = torch.autograd.grad(torch.clip(xa, -c, c), xa, gs)
    assert torch.equal(got.cpu(), ga)
    # one row alone: same numbers whatever the batch (and, for odd L, on the other load path)
    r1, mask1, part1 = clip_residual(xd[:1], yd[:1], c)
    assert torch.equal(r1, r[:1]) and torch.equal(mask1, mask[:1]) and torch.equal(part1, part[:1])
    assert torch.equal(deg.fwd(xd[:1]), deg.fwd(xd)[:1])
    deg.residual(xd[:1], yd[:1])
    assert torch.equal(deg.adj(gd[:1]), got[:1])


def test_clip_degradation_guidance_is_the_masked_seed():
    from babe_amd.degrade import ClipDegradation
    c, x, y, gs, xd, yd, gd = _clip_case(1003)
    deg = ClipDegradation(c)
    got = deg.guidance(xd, yd, lambda r, yy, part, post: r)
    assert torch.equal(got.cpu(), (y - torch.clip(x, -c, c)) * (x.abs() <= c))


# ---- STFT magnitude -------------------------------------------------------------------------------------------------------
STFT_CASES = [(256, 64, 1000), (1024, 256, 5000), (4096, 1024, 9001), (256, 64, 100), (512, 512, 2048)]


def _stft_mag64(x, win, hop):
    xp = torch.cat((x, torch.zeros(x.shape[0], win, dtype=x.dtype)), -1)
    X = torch.stft(xp, win, hop_length=hop, window=torch.hamming_window(win, dtype=torch.float32).to(x.dtype), center=False,
                   return_complex=True)
    return torch.sqrt(X.real ** 2 + X.imag ** 2), X


_ref_cache = {}


def _stft_ref(win, hop, L, zero_row=False):
    """(x, G, float64 magnitude, float64 autograd VJP with NaN -> 0): computed once per case and left unchanged."""
    key = (win, hop, L, zero_row)
    if key not in _ref_cache:
        g = torch.Generator().manual_seed(win + hop + L)
        x = torch.randn(2, L, generator=g)
        if zero_row:
            x[1] = 0
        bins, frames = win // 2 + 1, 1 + L // hop
        Gs = torch.randn(2, bins, frames, generator=g)
        xa = x.double().requires_grad_(True)
        mag, _ = _stft_mag64(xa, win, hop)
        assert mag.shape == (2, bins, frames)
        gx, = torch.autograd.grad(mag, xa, Gs.double())
        _ref_cache[key] = (x, Gs, mag.detach(), torch.nan_to_num(gx, nan=0.0), bool(torch.isnan(gx).any()))
    return _ref_cache[key]


@pytest.mark.parametrize("win,hop,L", STFT_CASES)
def test_stft_magnitude_forward_and_vjp_vs_float64_torch(win, hop, L):
    from babe_amd.degrade import STFTMagnitudeDegradation
    x, Gs, mag, gx, had_nan = _stft_ref(win, hop, L)
    deg = STFTMagnitudeDegradation(win, hop, L, "cuda")
    out = deg.fwd(x.cuda())
    assert out.shape == (2, mag.shape[1] * mag.shape[2]) and deg.out_shape() == tuple(mag.shape[1:])
    e_f = row_rel(out, mag)
    got = deg.adj(Gs.cuda().reshape(2, -1))
    assert got.shape == (2, L) and bool(torch.isfinite(got).all())
    e_b = row_rel(got, gx)
    print(f"stft_mag ({win}, {hop}, {L}): forward {e_f:.2e}, vjp {e_b:.2e} (relative, worst row); torch NaN: {had_nan}")
    assert e_f < TOL and e_b < TOL
    if L % hop == 0:
        assert bool((out.reshape(2, -1, 1 + L // hop)[:, :, -1] == 0).all())


def test_stft_magnitude_of_an_all_zero_row_has_a_zero_vjp():
    from babe_amd.degrade import STFTMagnitudeDegradation
    win, hop, L = 256, 64, 1000
    x, Gs, mag, gx, had_nan = _stft_ref(win, hop, L, zero_row=True)
    assert had_nan
    deg = STFTMagnitudeDegradation(win, hop, L, "cuda")
    out = deg.fwd(x.cuda())
    got = deg.adj(Gs.cuda().reshape(2, -1))
    assert bool(torch.isfinite(got).all()) and bool((out[1] == 0).all()) and bool((got[1] == 0).all())
    assert row_rel(out[:1], mag[:1]) < TOL and row_rel(got[:1], gx[:1]) < TOL


@pytest.mark.parametrize("win,hop,L", [(256, 64, 1000), (1024, 1000, 5000)])
def test_stft_magnitude_vjp_is_the_adjoint_of_the_frozen_phasor_path(win, hop, L):
    """With the phasors U = X / |X| frozen at a fixed x, x' -> Re(conj(U) STFT(x')) is linear and the VJP is its transpose:
    <Re(conj(U) STFT(x')), G> == <x', vjp(G)> to 1e-6, the left side and both sums in float64 on the host."""
    from babe_amd.degrade import STFTMagnitudeDegradation
    x, Gs, _, _, _ = _stft_ref(win, hop, L)
    deg = STFTMagnitudeDegradation(win, hop, L, "cuda")
    deg.fwd(x.cuda())
    U = torch.view_as_complex(deg.spec.cpu().double().contiguous())             # [B][frames][bins], the GPU's own spectrum
    U = torch.where(U.abs() > 0, U / U.abs().clamp_min(1e-300), torch.zeros_like(U)).transpose(1, 2)
    xp = torch.randn(2, L, generator=torch.Generator().manual_seed(5)).double()
    _, Xp = _stft_mag64(xp, win, hop)
    lhs = ((U.conj() * Xp).real * Gs.double()).sum(dim=(1, 2))
    rhs = (xp * deg.adj(Gs.cuda().reshape(2, -1)).cpu().double()).sum(dim=1)
    err = float(((lhs - rhs).abs() / lhs.abs()).max())
    print(f"adjoint identity ({win}, {hop}, {L}): {err:.2e}")
    assert err < 1e-6


def test_stft_magnitude_is_deterministic_and_independent_of_the_batch():
    from babe_amd.degrade import STFTMagnitudeDegradation
    win, hop, L = 1024, 256, 5000
    x, Gs, _, _, _ = _stft_ref(win, hop, L)
    xd, gd = x.cuda(), Gs.cuda().reshape(2, -1)
    deg = STFTMagnitudeDegradation(win, hop, L, "cuda")
    a, ga = deg.fwd(xd), deg.adj(gd)
    b, gb = deg.fwd(xd), deg.adj(gd)
    assert torch.equal(a, b) and torch.equal(ga, gb)
    one, g1 = deg.fwd(xd[:1]), deg.adj(gd[:1])
    assert torch.equal(one, a[:1]) and torch.equal(g1, ga[:1])


# ---- matrix 2-norm seed ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", [(129, 16), (513, 20), (129, 150), (2049, 5)])
def test_specnorm_seed_is_torchs_gradient_of_the_matrix_2_norm(rows, cols):
    """-u1 v1^T against float64 autograd of torch.linalg.norm(y - rec, dim=(1, 2), ord=2), 1e-5 relative per row.  R = 1 + 0.5 N(0, 1):
    s2 / s1 is about 0.5 (1 / sqrt(rows) + 1 / sqrt(cols)) <= 0.3 here, so 32 iterations are converged to float32.  Fewer than 64
    columns, more than 64, rows no multiple of 4; a zero residual gives exactly 0."""
    from babe_amd.degrade import specnorm_seed
    g = torch.Generator().manual_seed(rows + cols)
    R = 1.0 + 0.5 * torch.randn(2, rows, cols, generator=g)
    R[1] = -R[1]
    rec = torch.zeros(2, rows, cols, dtype=torch.float64, requires_grad=True)
    want, = torch.autograd.grad(torch.linalg.norm(R.double() - rec, dim=(1, 2), ord=2).sum(), rec)
    sv = torch.linalg.svdvals(R.double())
    assert float((sv[:, 1] / sv[:, 0]).max()) < 0.5
    rd = R.reshape(2, -1).cuda()
    got = specnorm_seed(rd, rows, cols)
    err = row_rel(got, want)
    print(f"specnorm_seed ({rows}, {cols}): {err:.2e} (relative, worst row)")
    assert err < TOL
    assert torch.equal(specnorm_seed(rd, rows, cols), got) and torch.equal(specnorm_seed(rd[:1], rows, cols), got[:1])
    z = rd.clone()
    z[1] = 0
    gz = specnorm_seed(z, rows, cols)
    assert torch.equal(gz[0], got[0]) and bool((gz[1] == 0).all())


def test_stft_magnitude_guidance_with_the_matrix_norm_ignores_the_seed_and_chains_the_vjp():
    from babe_amd.degrade import STFTMagnitudeDegradation, specnorm_seed
    win, hop, L = 256, 64, 1000
    x, _, mag, _, _ = _stft_ref(win, hop, L)
    y = (0.5 * mag.float()).reshape(2, -1).cuda()
    deg = STFTMagnitudeDegradation(win, hop, L, "cuda", matrix_norm=True)
    got = deg.guidance(x.cuda(), y, None)
    plain = STFTMagnitudeDegradation(win, hop, L, "cuda")
    r = y - plain.fwd(x.cuda())
    assert torch.equal(got, plain.adj(specnorm_seed(r, *plain.out_shape())))
    xa = x.double().requires_grad_(True)
    want, = torch.autograd.grad(torch.linalg.norm(0.5 * mag - _stft_mag64(xa, win, hop)[0], dim=(1, 2), ord=2).sum(), xa)
    err = row_rel(got, want)
    print(f"matrix-norm guidance: {err:.2e}")
    assert err < TOL


# ---- samplers -------------------------------------------------------------------------------------------------------------
class ResidualNet:
    """The wrapper of tests/golden/make_golden.py (as in test_gpu_sampler.py): a*net(x,c) + (sigma/sigma_data)*x, sigma = exp(4c)."""

    def __init__(self, inner, a, sigma_data):
        self.inner, self.a, self.sd = inner, a, sigma_data
        self.CQTransform = inner.CQTransform

    def fwd_nograd(self, x, cn):
        self.k = float(torch.exp(4 * cn[0, 0])) / self.sd
        return self.a * self.inner.fwd_nograd(x, cn) + self.k * x

    def vjp(self, g):
        return self.a * self.inner.vjp(g) + self.k * g


_net_cache = {}


def _setup(fx, rid=True, **over):
    from babe_amd.config import default_args
    from babe_amd.diff_params.edm import EDM
    from babe_amd.networks.cqtdiff_plus import Unet_CQT_oct_with_attention
    from babe_amd.testing.edm_sampler import Sampler
    args = default_args(sample_rate=22050, audio_len=92092, Ns=[8, 8, 8, 8, 16, 16, 16], T=3, start_sigma=0.05)
    if "net" not in _net_cache:
        g = load("unet_small.npz")
        net = Unet_CQT_oct_with_attention(args, "cuda")
        net.load_state_dict({k[3:]: v for k, v in g.items() if k.startswith("sd.")}, strict=True)
        _net_cache["net"] = net
    args.tester.posterior_sampling.xi = over.get("xi", float(fx["xi"]))
    args.tester.posterior_sampling.data_consistency = over.get("data_consistency", False)
    args.tester.diff_params.ro = float(fx["ro"])
    args.tester.diff_params.sigma_max = float(fx["sigma_max"])
    args.tester.diff_params.Schurn = float(fx["Schurn"])
    return Sampler(ResidualNet(_net_cache["net"], float(fx["res_a"]), 0.063), EDM(args), args, rid=rid)


def _signals(fx, L=92092):
    """The fixture script's signals(): clean signal, the four recorded noises, the compressed-sensing mask, in that order."""
    g = torch.Generator().manual_seed(int(fx["seed"]))
    clean = 0.1 * torch.randn(1, L, generator=g)
    noises = [torch.randn(1, L, generator=g) for _ in range(4)]
    mask = (torch.rand(1, L, generator=g) < float(fx["keep"])).float()
    return clean, noises, mask


def _with_noises(smp, noises):
    it = iter(noises)
    smp._randn = lambda shape, device: next(it).to(device)
    return smp


def _check(task, fx, out):
    """The bars of test_gpu_sampler.py::test_edm_sampler_inpainting_T3_vs_reference_golden on the final x, and the same on
    the state after every step; t equal."""
    x, den, t = out
    xs, ds = int(fx["x_stride"]), int(fx["stride"])
    xr, dr = fx[f"{task}_x"], fx[f"{task}_den"]
    ex, rx = rms_err(x[:, ::xs], xr), rel(x[:, ::xs], xr)
    ed, rd = rms_err(den[..., ::ds], dr), rel(den[..., ::ds], dr)
    print(f"{task}: final x RMS err {ex:.2e}, rel {rx:.2e}; per-step states RMS err {ed:.2e}, rel {rd:.2e}")
    assert torch.equal(torch.as_tensor(t).float().cpu(), fx["t"].float())
    assert ex < 1e-3 and rx < 2e-3
    assert ed < 1e-3 and rd < 2e-3


def test_declipping_T3_vs_reference_golden():
    fx = load("edm_sampler_tasks.npz")
    clean, noises, _ = _signals(fx)
    c = float(fx["clip_value"])
    smp = _with_noises(_setup(fx), noises)
    _check("declip", fx, smp.predict_declipping(torch.clip(clean, -c, c).cuda(), c))
    assert smp.degradation is None


def test_compsens_T3_vs_reference_golden_and_equals_inpainting():
    fx = load("edm_sampler_tasks.npz")
    clean, noises, mask = _signals(fx)
    y = (mask * clean).cuda()
    smp = _with_noises(_setup(fx), noises)
    out = smp.predict_compsens(y, mask)
    _check("compsens", fx, out)
    same = _with_noises(_setup(fx), noises).predict_inpainting(y, mask)
    assert torch.equal(out[0], same[0]) and torch.equal(out[1], same[1])


def test_phase_retrieval_T3_vs_reference_golden():
    """The reference's guidance for its 3-D observation is the matrix 2-norm of the residual (largest singular value):
    predict_pr differentiates that, for a 3-D and for a flattened y alike.  The bars of the inpainting fixture; the reference's
    own float32-against-float64 spread on this run is 4.9e-5 RMS / 4.5e-5 relative (fixture script, --spread)."""
    fx = load("edm_sampler_tasks.npz")
    clean, noises, _ = _signals(fx)
    win, hop = int(fx["win"]), int(fx["hop"])
    y, _ = _stft_mag64(clean, win, hop)
    smp = _with_noises(_setup(fx), noises)
    out = smp.predict_pr(y.cuda(), win, hop)
    _check("pr", fx, out)
    assert smp.degradation is None
    flat = _with_noises(_setup(fx, rid=False), noises).predict_pr(y.reshape(1, -1).cuda())      # flattened y, YAML-less defaults
    assert torch.equal(flat, out[0])


def test_task_refusals_with_a_live_network():
    fx = load("edm_sampler_tasks.npz")
    y = torch.zeros(1, 92092, device="cuda")
    for kw, exc in ((dict(xi=0.0), ValueError), (dict(data_consistency=True), ValueError)):
        smp = _setup(fx, **kw)
        with pytest.raises(exc):
            smp.predict_declipping(y, 0.1)
        with pytest.raises(exc):
            smp.predict_compsens(y, torch.ones(92092))
    with pytest.raises(NotImplementedError, match="data_consistency"):
        _setup(fx, data_consistency=True).predict_pr(torch.zeros(1, 513, 360, device="cuda"))
    with pytest.raises(ValueError, match="xi"):
        _setup(fx, xi=0.0).predict_pr(torch.zeros(1, 513, 360, device="cuda"))
    with pytest.raises(ValueError, match="513, 360"):
        _setup(fx).predict_pr(torch.zeros(1, 513, 361, device="cuda"))
