"""The kernels of csrc/stft.hip element by element against float64 references, at the sizes, strides and flag sets where they can
go wrong: every transform size 256...4096, one-frame and all-zero-frame lengths, strided rows, per-clip filters, the `pre` and
`part` arguments, and ONE step of the projected-gradient fit on both kernels for every K, weighting and clamp switch.  Cases and
references: tests/stft_cases.py (pinned on the CPU by tests/test_stft_cases_cpu.py).  Needs a MI355X.

Metric: max|got - ref| / max|ref| per clip, and per frame for framed results (stft_cases.framed_err / sample_err); where the
reference is exactly zero the result must be exactly zero.

Bars.  Ceilings are the project's existing bars (5e-6 for the transforms, tests/fft_cases.py; 2e-5 / 5e-4 for the fit's loss /
gradient, 3e-6 for H and 2e-5 for the distance gradient, tests/test_gpu_stft.py and test_gpu_sampler.py).  Each bar below is four
times the largest error measured on a MI355X over every case of this file against the float64 references (a max-norm moves that
much from seed to seed), capped at its ceiling:
  quantity                                           measured max   bar
  spectra (stft)                                     3.50e-7        1.4e-6
  filtered frames (filter_frames)                    1.91e-7        7.7e-7
  overlap-added samples, residuals, whole chain      9.03e-7        3.7e-6
  residual seed                                      4.27e-7        1.8e-6
  partial sums of squares (float64 accumulation)     4.1e-16        1e-12 (stated, not measured: double rounding)
  per-bin statistics                                 1.34e-7        3.0e-7 (derived, 5 u: test_mag_stats_per_bin)
  distance gradient, per clip                        6.17e-7        2.5e-6
  H of design_filter, relative per bin               1.35e-6        3e-6 (the ceiling)
  fit loss (babe_filter_loss_grad)                   1.11e-7        4.5e-7
  fit gradient, reference-order kernel               8.47e-7        3.4e-6
  fit gradient, fast kernel                          1.46e-6        5.9e-6
For comparison, the oracle's own float32 step is within 1e-6 (gradient) and 1.1e-7 (loss) of float64 on these cases.  The fast
kernel's bar is above the reference-order kernel's because it evaluates the segments as exp2(P log2 f + Q) on the hardware's
v_exp_f32 / v_log_f32 (1 ulp each, and the rounding of log2 f is multiplied by P) and forms 1 / loss in float32.  In the
one-step test the bound mu * bar * max|g| + 2 ulp is dominated by the 2 ulp on every case (measured excess over 2 ulp: none).
"""
import pytest
import torch

from oracle import bwe_utils as U
from tests import stft_cases as sc

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24                                  # unit roundoff of float32
STFT_BAR = 1.4e-6                                 # spectra
FRAMES_BAR = 7.7e-7                               # filtered, windowed frames
OLA_BAR = 3.7e-6                                  # overlap-added samples, residuals, the analysis-synthesis chain
SEED_BAR = 1.8e-6                                 # residual seeds
SUMSQ_BAR = 1e-12                                 # float64 accumulation of the kernel's own float32 residual
STATS_BAR = 5 * U32                               # see test_mag_stats_per_bin
DIST_BAR = 2.5e-6                                 # distance gradient
DESIGN_BAR = 3e-6                                 # H, relative per bin (the bar of test_design_filter_vs_golden)
LOSS_BAR = 4.5e-7                                 # fit loss, relative
GRAD_BAR = {0: 5.9e-6, 1: 3.4e-6}                    # fit gradient relative to its row's maximum: fast kernel, reference-order kernel

TIDS = [sc.transform_id(c) for c in sc.TRANSFORM_CASES]
FIT_NAMES = [c["name"] for c in sc.FIT_CASES]


def _rec(quantity, value):
    print(f"STFT_EDGE {quantity} {value:.3e}")
    return value


# ----------------------------------------------------------------------------- 3. transforms and overlap-add
@pytest.mark.parametrize("c", sc.TRANSFORM_CASES, ids=TIDS)
def test_stft_per_frame_and_bin(c):
    nfft, L = c[:2]
    x = sc.transform_inputs(nfft, L)[0]
    d = sc.Direct(nfft, L)
    spec = d.stft(x)
    assert spec.shape == (x.shape[0], sc.n_frames(L, nfft), nfft // 2 + 1, 2)
    assert _rec("stft", sc.framed_err(sc.as_complex(spec), sc.stft64(x, nfft))) < STFT_BAR


@pytest.mark.parametrize("c", sc.TRANSFORM_CASES, ids=TIDS)
def test_stft_pre_multiplies_the_signal_first(c):
    """babe_stft_fwd's `pre` (exported, passed by no caller): bit-identical to the STFT of x * pre[:L] formed on the device."""
    nfft, L = c[:2]
    x = sc.transform_inputs(nfft, L)[0]
    d = sc.Direct(nfft, L)
    got = d.stft(x, pre=True)
    want = d.stft((x.cuda() * d.st.env_inv[:L]).cpu())
    assert not bool(torch.isnan(got).any()) and torch.equal(got, want)
    assert not torch.equal(got, d.stft(x))


@pytest.mark.parametrize("c", sc.TRANSFORM_CASES, ids=TIDS)
def test_filter_frames_of_a_random_spectrum_per_frame(c):
    """w * irfft(spec * H) of a spectrum that is NOT the transform of a real signal, with one filter for the batch, with a filter
    per clip (distinct rows), and with every entry of H zero but DC / but Nyquist (the two bins the kernel treats apart)."""
    nfft, L = c[:2]
    _, _, spec, H = sc.transform_inputs(nfft, L)
    d = sc.Direct(nfft, L)
    Z = sc.as_complex(spec)
    e_dc, e_ny = torch.zeros(nfft // 2 + 1), torch.zeros(nfft // 2 + 1)
    e_dc[0], e_ny[-1] = 1.5, 0.75
    for what, h in (("shared", H[0].contiguous()), ("per-clip", H), ("dc-only", e_dc), ("nyquist-only", e_ny)):
        err = _rec("frames", sc.framed_err(d.filter_frames(spec, h).double(), sc.filtered_frames64(Z, h, nfft)))
        assert err < FRAMES_BAR, (what, err)


@pytest.mark.parametrize("nfft,L", [(256, 389), (512, 773), (4096, 6149)])
def test_filter_frames_ignores_the_imaginary_parts_at_dc_and_nyquist(nfft, L):
    """irfft ignores them: the frames of a spectrum are BIT-identical to the frames of the same spectrum with those two imaginary
    parts set to zero.  (In fft_lds_inplace the slots of DC and Nyquist lie in the first block, which no pass multiplies by a
    twiddle, so an imaginary part stored there reaches imaginary outputs only: the kernel's `k == 0 || k == hop` branch is a
    statement of intent, and this test holds the property whichever way it is met.)"""
    _, _, spec, H = sc.transform_inputs(nfft, L)
    assert float(spec[:, :, 0, 1].abs().min()) > 0 and float(spec[:, :, -1, 1].abs().min()) > 0
    clean = spec.clone()
    clean[:, :, 0, 1] = 0
    clean[:, :, -1, 1] = 0
    d = sc.Direct(nfft, L)
    assert torch.equal(d.filter_frames(spec, H), d.filter_frames(clean, H))


@pytest.mark.parametrize("c", sc.TRANSFORM_CASES, ids=TIDS)
def test_ola_per_sample(c):
    """Overlap-add of random float32 frames, plain and normalised; residual mode out = y - ola with the partial sums of squares
    against the float64 sum over the kernel's OWN float32 residual (a float64 accumulation: 1e-12 relative)."""
    nfft, L = c[:2]
    x, y, _, _ = sc.transform_inputs(nfft, L)
    T = sc.n_frames(L, nfft)
    fr = torch.randn(x.shape[0], T, nfft, generator=torch.Generator().manual_seed(L))
    d = sc.Direct(nfft, L)
    env = sc.env_inv64(nfft, T)
    assert _rec("ola", sc.sample_err(d.ola(fr, False).double(), sc.ola64(fr, L))) < OLA_BAR
    assert _rec("ola", sc.sample_err(d.ola(fr, True).double(), sc.ola64(fr, L, env))) < OLA_BAR
    for normalise in (False, True):
        r, part = d.ola(fr, normalise, y=y)
        rref, _ = sc.ola64(fr, L, env if normalise else None, y=y)
        assert _rec("ola", sc.sample_err(r.double(), rref)) < OLA_BAR
        assert part.shape == (x.shape[0], d.nblk) and bool((part >= 0).all())
        own = (r.double() ** 2).sum(1)
        assert _rec("sumsq", float(((part.sum(1) - own).abs() / own).max())) < SUMSQ_BAR


def test_analysis_filter_synthesis_chain_at_every_size():
    """stft -> filter_frames -> normalised ola on the device against the float64 chain, per sample: the first hop (one frame
    only) and the last L % hop samples weigh as much as any other."""
    for nfft, L, _ in sc.TRANSFORM_CASES:
        x, _, _, H = sc.transform_inputs(nfft, L)
        d = sc.Direct(nfft, L)
        got = d.ola(d.filter_frames(d.stft(x), H), True)
        ref = sc.ola64(sc.filtered_frames64(sc.stft64(x, nfft), H, nfft), L, sc.env_inv64(nfft, sc.n_frames(L, nfft)))
        hop = nfft // 2
        for what, sl in (("all", slice(None)), ("first hop", slice(0, min(hop, L))), ("tail", slice(L - max(L % hop, 1), L))):
            err = _rec("chain", sc.sample_err(got[:, sl].double(), ref[:, sl]))
            assert err < OLA_BAR, (nfft, L, what, err)


def test_strided_rows_of_x_y_and_the_ola_output():
    """x, y and the overlap-add output as rows of [B][L + 7] buffers: bit-identical to the contiguous calls (which the tests above
    hold to the references), nothing written between the rows."""
    nfft, L = 256, 1000
    x, y, _, H = sc.transform_inputs(nfft, L)
    d = sc.Direct(nfft, L)
    stride = L + sc.STRIDE_PAD
    spec = d.stft(x)
    assert torch.equal(d.stft(x, stride=stride), spec)
    fr = d.filter_frames(spec, H)
    r, part = d.ola(fr, True, y=y)
    rs, parts = d.ola(fr, True, y=y, stride=stride)
    assert torch.equal(rs, r) and torch.equal(parts, part)
    assert torch.equal(d.ola(fr, False, stride=stride), d.ola(fr, False))
    assert sc.sample_err(r.double(), sc.ola64(fr, L, sc.env_inv64(nfft, d.T), y=y)[0]) < OLA_BAR


@pytest.mark.parametrize("post", [True, False])
def test_residual_seed_per_sample(post):
    """-r / |r| * post per sample from the partial sums of |r|^2; a residual that is zero throughout (clip 1) gives zeros."""
    nfft, L = 256, 1000
    g = torch.Generator().manual_seed(9)
    r = 0.1 * torch.randn(3, L, generator=g)
    r[1] = 0
    d = sc.Direct(nfft, L)
    ss = (r.double() ** 2).sum(1)
    part = (ss[:, None] * torch.softmax(torch.randn(3, d.nblk, generator=g).double(), 1)).contiguous()
    got = d.residual_seed(r, part, post)
    ref = -r.double() / torch.where(ss > 0, ss.sqrt(), torch.ones_like(ss))[:, None]
    if post:
        ref = ref * sc.env_inv64(nfft, d.T)[:L]
    assert not bool(torch.isnan(got).any()) and bool((got[1] == 0).all())
    assert _rec("seed", sc.sample_err(got.double(), ref)) < SEED_BAR


@pytest.mark.parametrize("nfft,L", [(256, 1000), (1024, 1541)])
@pytest.mark.parametrize("shared", [True, False])
def test_mag_stats_per_bin(nfft, L, shared):
    """sum |X|^2, sum |X||Y|, sum |Y|^2 per bin over the frames (and the batch if shared) of random float32 spectra, B = 3, against
    float64 on the same float32 numbers.  The kernel forms |X| = sqrtf(re^2 + im^2) in float32: the radicand carries 2 u (u from
    the squares, u from their sum), the correctly rounded root halves that to u and adds its own u, so each magnitude is within
    2 u, each product of two magnitudes within 4 u, and a sum of non-negative terms keeps the relative error of its terms; the
    products and the sums themselves are float64.  Bar: 5 u = 3.0e-7 per bin, relative (u = 2^-24; the fifth u covers the
    second-order terms)."""
    B = 3
    X, Y = (sc.transform_inputs(nfft, L, B=B, seed=s)[2] for s in (1, 2))
    d = sc.Direct(nfft, L)
    got = d.mag_stats(X, Y, shared)
    ref = sc.stats64(sc.as_complex(X), sc.as_complex(Y), shared)
    assert got.shape == ref.shape == (1 if shared else B, 3, nfft // 2 + 1)
    assert _rec("stats", float(((got - ref).abs() / ref).max())) < STATS_BAR


@pytest.mark.parametrize("mode", [0, 1])
def test_distance_grad_per_clip(mode):
    """distance_grad(shared=False): one distance per clip, so the gradient of clip b is that of the oracle's stft_distance on clip b
    alone, whatever the other clip's scale (clip 1 is 30 times louder).  Float64 autograd, max-norm per clip."""
    from babe_amd.stft import STFTOps, freq_weights
    nfft, L = 256, 1000
    rec, y, _, _ = sc.transform_inputs(nfft, L)
    rec[1] *= 30.0
    y[1] *= 30.0
    st = STFTOps(nfft, L, sc.FS, "cuda")
    got = st.distance_grad(rec.cuda(), y.cuda(), freq_weights(st.nbins, "sqrt").cuda(), mode, shared=False).double().cpu()
    ref = torch.zeros(2, L, dtype=torch.float64)
    for b in range(2):
        q = rec[b:b + 1].double().requires_grad_(True)
        ref[b], = torch.autograd.grad(U.stft_distance(y[b:b + 1].double(), q, nfft, weight="sqrt", mag=mode == 1), q)
    assert _rec("dist", sc.sample_err(got, ref)) < DIST_BAR
    shared = st.distance_grad(rec.cuda(), y.cuda(), freq_weights(st.nbins, "sqrt").cuda(), mode, shared=True).double().cpu()
    assert sc.sample_err(shared[:1], ref[:1]) > 0.5                       # (the coupled distance is another gradient)


@pytest.mark.parametrize("nfft,L", [(256, 1000), (512, 773)])
def test_batch_rows_are_independent_and_calls_repeat_bit_for_bit(nfft, L):
    from babe_amd.stft import STFTOps
    x, _, spec, H = (t.cuda() for t in sc.transform_inputs(nfft, L, B=3))
    st = STFTOps(nfft, L, sc.FS, "cuda")
    fr = st.filter_frames(spec, H)
    calls = {"stft": lambda s: st.stft(x[s]), "filter_frames": lambda s: st.filter_frames(spec[s], H[s]),
             "ola": lambda s: st.ola(fr[s], True)}
    for name, f in calls.items():
        full, again = f(slice(0, 3)), f(slice(0, 3))
        assert not bool(torch.isnan(full).any()) and torch.equal(full, again), f"{name}: two identical calls differ"
        for b in range(3):
            assert torch.equal(f(slice(b, b + 1))[0], full[b]), f"{name}: row {b} of B = 3 differs from its B = 1 call"


# ----------------------------------------------------------------------------- 4. one step of the fit, both kernels
def _implied(dev, q, mu_j, gmax):
    """Gradient error, relative to the row's maximum, that a parameter deviation implies once 2 ulp are taken off."""
    return float(((dev - 2.0 * sc.ulp32(q)).clamp(min=0) / (mu_j * gmax)).max())


@pytest.mark.parametrize("kernel", [0, 1], ids=["fast", "reference-order"])
@pytest.mark.parametrize("name", FIT_NAMES)
def test_one_descent_step(name, kernel):
    """max_iter = 1: the updated parameters against fit_step64's within |d fc_j| <= mu_fc bar max|g_fc| + 2 ulp(fc_j) (likewise A),
    from the float64 gradient of the case; n_iter = 1; each row of a P = 3 launch bit-identical to its own P = 1 call."""
    c = sc.FIT_BY_NAME[name]
    stats, params, f, cfg = sc.fit_inputs(c)
    got, nit = sc.run_fit(stats, params, c["nfft"], c["fs"], cfg, kernel)
    P = params.shape[0]
    assert nit == [1] * P and not bool(torch.isnan(got).any())
    for p in range(P):
        _, g, q = sc.fit_step64(stats[p], params[p], f, cfg)
        dev = (got[p].double() - q).abs()
        for i in range(2):
            _rec(f"step-kernel{kernel}", _implied(dev[i], q[i], cfg["mu"][i], float(g[i].abs().max())))
        assert bool((dev <= sc.step_bounds(g, q, cfg["mu"], GRAD_BAR[kernel])).all()), (name, p, got[p], q)
        if P > 1:
            one, nit1 = sc.run_fit(stats[p:p + 1], params[p:p + 1], c["nfft"], c["fs"], cfg, kernel)
            assert nit1 == [1] and torch.equal(one[0], got[p]), f"row {p} of the P = {P} launch differs from its P = 1 call"


@pytest.mark.parametrize("name", FIT_NAMES)
def test_loss_and_gradient_kernel_on_the_one_step_cases(name):
    """babe_filter_loss_grad (the reference-order kernel, no step) at the same cases: loss and every gradient term."""
    from babe_amd.stft import STFTOps, make_fit_cfg
    c = sc.FIT_BY_NAME[name]
    stats, params, f, cfg = sc.fit_inputs(c)
    st = STFTOps(c["nfft"], c["nfft"], c["fs"], "cuda")
    lg = st.filter_loss_grad(stats.cuda(), params.cuda(), make_fit_cfg(**cfg)).double().cpu()
    K = c["K"]
    for p in range(params.shape[0]):
        loss, g, _ = sc.fit_step64(stats[p], params[p], f, cfg)
        assert _rec("loss", abs(float(lg[p, 0]) - loss) / loss) < LOSS_BAR
        for i in range(2):
            err = _rec("grad-kernel1", float((lg[p, 1 + i * K: 1 + (i + 1) * K] - g[i]).abs().max() / g[i].abs().max()))
            assert err < GRAD_BAR[1], (name, p, i, lg[p], g)


@pytest.mark.parametrize("kernel", [0, 1], ids=["fast", "reference-order"])
@pytest.mark.parametrize("K", sc.GRAD_KS)
def test_gradient_terms_read_off_an_unclamped_step(K, kernel):
    """clamp_fc = clamp_A = 0 and mu = (1, 1): p_old - p_new IS the gradient, up to the rounding of the stored parameter (half a
    float32 spacing, taken off; the statistics are scaled so that it is below a tenth of the ceiling).  Per parameter against
    fit_step64's gradient, relative to the row's maximum: a wrong suffix sum or anchor term Lj shows here."""
    stats, params, f, cfg = sc.grad_inputs(K)
    got, nit = sc.run_fit(stats, params, 4096, sc.FS, cfg, kernel)
    _, g, _ = sc.fit_step64(stats[0], params[0], f, cfg)
    old, new = params[0].double(), got[0].double()
    half = 0.5 * torch.maximum(sc.ulp32(old), sc.ulp32(new))
    assert nit == [1]
    for i in range(2):
        err = _rec(f"grad-kernel{kernel}", float((((old[i] - new[i]) - g[i]).abs() - half[i]).clamp(min=0).max() / g[i].abs().max()))
        assert err < GRAD_BAR[kernel], (K, i, old[i] - new[i], g[i])


@pytest.mark.parametrize("kernel", [0, 1], ids=["fast", "reference-order"])
def test_fit_stops_in_two_iterations_at_the_exact_parameters(kernel):
    """Statistics with Y = X H(p*), started at p* under the default mu and tolerances (stft_cases.exact_inputs bounds every step
    by tol / 8): the first iteration cannot stop (nothing to compare with), the second does; the parameters stay within the
    tolerance of p*."""
    stats, params, f, cfg = sc.exact_inputs()
    got, nit = sc.run_fit(stats, params, 4096, sc.FS, cfg, kernel, max_iter=100)
    assert nit == [2], nit
    assert float((got[0, 0] - params[0, 0]).abs().max()) < 5e-3 and float((got[0, 1] - params[0, 1]).abs().max()) < 5e-3


@pytest.mark.parametrize("kernel", [0, 1], ids=["fast", "reference-order"])
def test_three_iterations_are_three_chained_single_iterations(kernel):
    """The state carried between iterations (the previous parameters of the stopping rule) changes no update: max_iter = 3 on a
    case that does not converge returns n_iter = 3 and the parameters of three max_iter = 1 calls, bit for bit."""
    c = sc.FIT_BY_NAME["K5-nfft4096"]
    stats, params, f, cfg = sc.fit_inputs(c)
    got, nit = sc.run_fit(stats, params, 4096, sc.FS, cfg, kernel, max_iter=3)
    assert nit == [3]
    p = params
    for _ in range(3):
        p, n1 = sc.run_fit(stats, p, 4096, sc.FS, cfg, kernel, max_iter=1)
        assert n1 == [1]
    assert torch.equal(p, got) and not torch.equal(got, params)


@pytest.mark.parametrize("nfft", [256, 4096])
@pytest.mark.parametrize("name", list(sc.DESIGN_CASES))
def test_design_filter_rows(name, nfft):
    """Against the oracle in float64 on the float32 frequencies; the pass-band masks coincide exactly.  The unsorted rows reach the
    "older value" search of build_filter."""
    from babe_amd.stft import STFTOps
    st = STFTOps(nfft, nfft, sc.FS, "cuda")
    p = torch.tensor(sc.DESIGN_CASES[name])
    H = st.design_filter(p.cuda()).double().cpu()
    Href = U.design_filter(p[0].double(), p[1].double(), U.bin_freqs(nfft, sc.FS).double())
    assert torch.equal(H == 1.0, Href == 1.0)
    assert _rec("design", float(((H - Href).abs() / Href).max())) < DESIGN_BAR


# ----------------------------------------------------------------------------- 5. operands the wrappers must refuse
def test_wrappers_refuse_non_contiguous_operands():
    from babe_amd.stft import STFTOps, freq_weights
    nfft, L = 256, 1000
    st = STFTOps(nfft, L, sc.FS, "cuda")
    x, y, spec, H = (t.cuda() for t in sc.transform_inputs(nfft, L))
    permuted = spec.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)           # same shape and values, bins-major memory
    assert permuted.shape == spec.shape and not permuted.is_contiguous()
    every_other = torch.stack([H, H], -1)[..., 0]                                  # [B, nbins] with stride(-1) = 2
    w = freq_weights(st.nbins, "sqrt").cuda()
    with pytest.raises(AssertionError):
        st.filter_frames(permuted, H)
    with pytest.raises(AssertionError):
        st.filter_frames(spec, every_other)
    with pytest.raises(AssertionError):
        st.mag_stats(permuted, spec)
    with pytest.raises(AssertionError):
        st.mag_stats(spec, permuted)
    with pytest.raises(AssertionError):
        st.distance_grad(x, y, torch.stack([w, w], -1)[:, 0], 0)
    torch.cuda.synchronize()
