"""The CQT band and gather kernels (csrc/cqt.hip: band_fft_kernel, gather_rec_kernel, gather_kernel, spec_scale_kernel) and their
sequencing (babe_amd/cqt.py, csrc/cqt_plan.hip), per band and per clip against float64 references on small designs that reach
every band length 4 .. 4096, the wrapped and mirrored bands, both gather forms, the window-table kernels, the long Kaiser
polynomial and B >= 8.  Cases and references: tests/cqt_cases.py (pinned on the CPU by tests/test_cqt_cases_cpu.py).
Needs a MI355X."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import cqt_cases as cc

pytestmark = pytest.mark.gpu
IDS = list(cc.CASES)
CSR_CASES = [c for c in IDS if cc.CASES[c]["max_sources"] > 3]
U = 2.0 ** -24

# Band stages: at most three radix-16 passes and one window multiply in fp32.  Largest per-band error (max|got - ref| / max|ref|
# over the band's T coefficients or M spectrum entries) against the float64 references on a MI355X, max over both window kinds:
#   B = 2 (test_analysis_per_band / test_synthesis_per_band)
#     analysis    tiny 1.10e-7  short 2.08e-7  long 2.11e-7  deg7 2.16e-7  table 1.71e-7  rec9 1.74e-7
#     synthesis   tiny 1.35e-7  short 2.00e-7  long 2.09e-7  deg7 2.30e-7  table 2.00e-7  rec9 2.20e-7
#   B = 9 (test_nine_clips)                          analysis  rec9 2.20e-7  short 2.01e-7    synthesis  rec9 2.24e-7  short 2.55e-7
#   window from the table at beta = 1 (short)        analysis  1.67e-7                         synthesis  2.06e-7
# Each bar is four times the largest value of its stage, 2.20e-7 and 2.55e-7 (the factor covers the seed-to-seed spread of a
# max-norm); both stay below the bar the length-L transform meets (fft_cases.BAR = 5e-6).
ANALYSIS_BAR = 4 * 2.20e-7
SYNTHESIS_BAR = 4 * 2.55e-7
assert ANALYSIS_BAR <= cc.BAR and SYNTHESIS_BAR <= cc.BAR


def gather_bar(ref_abs, ref, sources):
    """Per clip.  A gather output is sc (v_1 + ... + v_S) with sc = fl(scale mul[n]): S - 1 rounded additions (the conjugate's
    sign is exact), one rounded product for sc and one for the result, so |error| <= (S + 1) u sc (|v_1| + ... + |v_S|) to first
    order, for the complex magnitude as well (Minkowski).  On the measure max|got - ref| / max|ref| that is (S + 1) u kappa with
    kappa = max_n sc sum|v_e| / max_n |ref| >= 1, computed from the inputs in float64 (`ref_abs`: the same gather of the entries'
    magnitudes), never from the kernel's output.  S = the largest source count of the case."""
    a = ref_abs.abs().reshape(ref_abs.shape[0], -1).max(1).values.numpy()
    r = np.hypot(ref[:, 0].numpy(), ref[:, 1].numpy()).reshape(ref.shape[0], -1).max(1)
    return (sources + 1) * U * a / r


# spec_scale: (s1 m) sc1 is two rounded products, a second source two more and one rounded addition (or an fma, which rounds less):
# |error| <= 3 u (|s1 m sc1| + |s2 m sc2|); with one source 2 u |ref|
SPEC_SCALE_ONE = 2 * U

_HIP = {}


def hip_of(case, c_plan="1", analytic="1"):
    """One CQT_nsgt per (case, BABE_CQT_C, BABE_CQT_ANALYTIC_WIN); both switches are read by the constructor only."""
    from babe_amd.cqt import CQT_nsgt
    key = (case, c_plan, analytic)
    if key not in _HIP:
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv("BABE_CQT_C", c_plan)
            mp.setenv("BABE_CQT_ANALYTIC_WIN", analytic)
            a, kw = cc.ctor(case)
            _HIP[key] = CQT_nsgt(*a, device="cuda", **kw)
    return _HIP[key]


def _ptr(t):
    return None if t is None else t.data_ptr()


def _kaiser_form(case, hip):
    want = cc.CASES[case]["kdeg"]
    if want is None:
        assert hip.kaiser is None, "beta = 6 has no polynomial of degree <= 11: the table kernels must run"
    else:
        assert hip.kaiser is not None and hip.kaiser[0] == want, (case, hip.kaiser)


# ----------------------------------------------------------------------------- stage calls on guarded buffers
def run_analysis(hip, case, spec, kind):
    """CQT_nsgt.analysis with the spectrum between NaN canaries and every coefficient tensor NaN-filled between canaries."""
    B = spec.shape[0]
    sp = cc.Guarded(spec.numel(), src=spec)
    out = cc.GuardedCoefs(case, B)
    win = hip.win_fwd if kind == "fwd" else hip.win_bwd_adj
    hip.analysis(sp.mid.view(B, 2, hip.fft.KX), win, out.views)
    torch.cuda.synchronize()
    assert sp.canaries_intact() and out.canaries_intact(), f"{case} {kind}: analysis wrote outside a buffer"
    return [v.cpu() for v in out.views]


def run_synthesis(hip, case, coefs, kind):
    """babe_cqt_band_synthesis the way CQT_nsgt.synthesis_spec calls it, band spectra NaN-filled between canaries."""
    from babe_amd._lib import lib, stream
    B = coefs[0].shape[0]
    inp = cc.GuardedCoefs(case, B, src=coefs)
    bs = cc.Guarded(B * hip.nwin * 2, canary=-3.0)
    win = hip.win_bwd if kind == "bwd" else hip.win_fwd_adj
    win = None if (win is hip.win_fwd_adj and hip.kaiser is not None) else win
    s = hip._bands(inp.views)
    rc = lib().babe_cqt_band_synthesis(C.byref(s), bs.mid.data_ptr(), _ptr(win), hip.nwin, B, stream())
    torch.cuda.synchronize()
    assert rc == 0, lib().babe_last_error()
    assert bs.canaries_intact() and inp.canaries_intact(), f"{case} {kind}: synthesis wrote outside a buffer (past nwin?)"
    return bs.mid.cpu().view(B, hip.nwin, 2)


def run_gather(hip, case, bs, scale, mul, use_rec):
    """babe_cqt_gather on guarded buffers; use_rec = False passes rec = NULL (the CSR kernel on the same data)."""
    from babe_amd._lib import lib, stream
    B, KX = bs.shape[0], hip.fft.KX
    inp = cc.Guarded(bs.numel(), src=bs)
    out = cc.Guarded(B * 2 * KX, canary=-3.0)
    mg = None if mul is None else cc.Guarded(mul.numel(), src=mul)
    rec = hip.rec if use_rec else None
    rc = lib().babe_cqt_gather(inp.mid.data_ptr(), hip.nwin, hip.rowptr.data_ptr(), hip.src.data_ptr(), _ptr(rec), out.mid.data_ptr(),
                               KX, hip.Ls, scale, None if mg is None else mg.mid.data_ptr(), B, stream())
    torch.cuda.synchronize()
    assert rc == 0, lib().babe_last_error()
    assert out.canaries_intact() and inp.canaries_intact(), f"{case}: gather wrote outside a buffer"
    return out.mid.cpu().view(B, 2, KX)


def run_spec_scale(hip, case, s1, mul, sc1, s2, sc2):
    from babe_amd._lib import lib, stream
    B, KX = s1.shape[0], hip.fft.KX
    g1 = cc.Guarded(s1.numel(), src=s1)
    g2 = None if s2 is None else cc.Guarded(s2.numel(), src=s2)
    mg = None if mul is None else cc.Guarded(mul.numel(), src=mul)
    out = cc.Guarded(B * 2 * KX, canary=-3.0)
    rc = lib().babe_spec_scale(g1.mid.data_ptr(), None if g2 is None else g2.mid.data_ptr(), out.mid.data_ptr(),
                               None if mg is None else mg.mid.data_ptr(), KX, hip.Ls, sc1, sc2, B, stream())
    torch.cuda.synchronize()
    assert rc == 0, lib().babe_last_error()
    assert out.canaries_intact(), f"{case}: spec_scale wrote outside its output"
    return out.mid.cpu().view(B, 2, KX)


def _zero_above(case, spec):
    """Every bin L/2 < n < KX compares equal to 0.0 (the buffer held NaN before the call)."""
    top = spec[:, :, cc.CASES[case]["L"] // 2 + 1:]
    return top.numel() > 0 and bool((top == 0.0).all())


def _gather_check(hip, case, B, seed, scale, with_mul, use_rec):
    bs = cc.rand_bs(case, B, seed)
    mul = cc.rand_mul(case, seed + 1) if with_mul else None
    got = run_gather(hip, case, bs, scale, mul, use_rec)
    ref = cc.ref_gather(case, bs, cc.f32(scale), mul)
    mag = torch.stack([torch.hypot(bs[..., 0].double(), bs[..., 1].double()), torch.zeros(bs.shape[:-1], dtype=torch.float64)], -1)
    bar = gather_bar(cc.ref_gather(case, mag, abs(cc.f32(scale)), mul)[:, 0], ref, cc.CASES[case]["max_sources"])
    err = cc.clip_err(got, ref, planar_axis=1)
    print(f"gather {case} B={B} scale={scale:g} mul={with_mul} {'records' if use_rec else 'CSR'}: err {err.max():.2e}  "
          f"bar {bar.min():.2e} = {cc.CASES[case]['max_sources'] + 1} u x kappa {bar.min() / ((cc.CASES[case]['max_sources'] + 1) * U):.2f}")
    assert _zero_above(case, got), f"{case}: gather left a bin above L/2 non-zero"
    assert bool((err < bar).all()), (case, err, bar)
    return got


def _spec_scale_check(hip, case, name, s1, m, a1, s2, a2):
    B, n = s1.shape[0], cc.CASES[case]["L"] // 2 + 1
    got = run_spec_scale(hip, case, s1, m, a1, s2, a2)
    ref = cc.ref_spec_scale(case, s1, m, cc.f32(a1), s2, cc.f32(a2))
    assert _zero_above(case, got), f"{case} {name}: spec_scale left a bin above L/2 non-zero"
    err = cc.clip_err(got, ref, planar_axis=1)
    if s2 is None:
        bar = np.full(B, SPEC_SCALE_ONE)
    else:                                                # 3 u kappa, kappa = max(|s1 m sc1| + |s2 m sc2|) / max|ref| from the inputs
        mm = torch.ones(n, dtype=torch.float64) if m is None else m.double()
        mag = lambda s: torch.hypot(s[:, 0, :n].double(), s[:, 1, :n].double())
        a = ((mag(s1) * abs(cc.f32(a1)) + mag(s2) * abs(cc.f32(a2))) * mm).max(1).values.numpy()
        bar = 3 * U * a / np.hypot(ref[:, 0].numpy(), ref[:, 1].numpy()).max(1)
    print(f"spec_scale {case} B={B} {name}: err {err.max():.2e}  bar {bar.min():.2e}")
    assert bool((err < bar).all()), (case, name, err, bar)
    return got


# ----------------------------------------------------------------------------- 1. analysis
@pytest.mark.parametrize("kind", cc.ANALYSIS_KINDS)
@pytest.mark.parametrize("case", IDS)
def test_analysis_per_band(case, kind):
    """Every band of every clip within the bar; the spectrum bins L/2 < n < KX hold NaN and must not be read; nothing outside
    the coefficient tensors is written.  fwd runs the analytic window where the design has one (degree 5, or 7 for beta = 2),
    bwd_adjoint's dual window always comes from the table."""
    hip = hip_of(case)
    _kaiser_form(case, hip)
    assert hip.win_bwd_adj is not hip.win_fwd                                   # analysis() takes the table form for it
    spec = cc.rand_spec(case, 2, cc.seed_of(case, 11))
    assert bool(torch.isnan(spec[:, :, cc.CASES[case]["L"] // 2 + 1:]).all())
    err = cc.coef_band_err(run_analysis(hip, case, spec, kind), cc.ref_analysis(case, spec, kind))
    print(f"analysis {case} {kind}: worst band {cc.worst(err):.2e} (band {int(np.nanargmax(err.max(0)))}), median {np.median(err):.2e}")
    assert bool((err < ANALYSIS_BAR).all()), (case, kind, np.argwhere(~(err < ANALYSIS_BAR))[:8], cc.worst(err))


# ----------------------------------------------------------------------------- 2. synthesis
@pytest.mark.parametrize("kind", cc.SYNTHESIS_KINDS)
@pytest.mark.parametrize("case", IDS)
def test_synthesis_per_band(case, kind):
    """Every one of the nwin band-spectrum entries is written (NaN before the call) and within the bar, per band; the canaries
    past nwin stay intact."""
    hip = hip_of(case)
    _kaiser_form(case, hip)
    assert hip.nwin == cc.geometry(case).nwin
    co = cc.rand_coefs(case, 2, cc.seed_of(case, 12))
    got = run_synthesis(hip, case, co, kind)
    assert not bool(torch.isnan(got).any()), f"{case} {kind}: {int(torch.isnan(got).sum())} band-spectrum values were not written"
    err = cc.bs_band_err(case, got, cc.ref_synthesis(case, co, kind))
    print(f"synthesis {case} {kind}: worst band {cc.worst(err):.2e} (band {int(np.nanargmax(err.max(0)))}), median {np.median(err):.2e}")
    assert bool((err < SYNTHESIS_BAR).all()), (case, kind, np.argwhere(~(err < SYNTHESIS_BAR))[:8], cc.worst(err))


# ----------------------------------------------------------------------------- 3. gather
@pytest.mark.parametrize("with_mul", [False, True], ids=["nomul", "mul"])
@pytest.mark.parametrize("case", IDS)
def test_gather_per_clip(case, with_mul):
    """Two scales; the designs with more than three sources on a bin have no record table (CSR kernel), the others run twice on
    the same data: with the records and with rec = NULL, which forces the CSR kernel."""
    hip = hip_of(case)
    if case in CSR_CASES:
        assert hip.rec is None
    else:
        assert hip.rec is not None and hip.rec.numel() == 4 * (hip.Ls // 2 + 1)
    for i, scale in enumerate((1.0, 2.0 / hip.Ls * 3.0)):
        for use_rec in ((True, False) if hip.rec is not None else (False,)):
            _gather_check(hip, case, 2, cc.seed_of(case, 20 + i), scale, with_mul, use_rec)


# ----------------------------------------------------------------------------- 4. spec_scale
@pytest.mark.parametrize("case", ["tiny", "long"])
def test_spec_scale(case):
    hip = hip_of(case)
    s1, s2 = cc.rand_spec(case, 2, cc.seed_of(case, 31)), cc.rand_spec(case, 2, cc.seed_of(case, 32))
    mul = cc.rand_mul(case, cc.seed_of(case, 33))
    _spec_scale_check(hip, case, "one source", s1, mul, 0.75, None, 0.0)
    _spec_scale_check(hip, case, "two sources", s1, mul, 0.75, s2, -1.5)
    _spec_scale_check(hip, case, "mul = None", s1, None, 1.25, s2, 0.3)
    _spec_scale_check(hip, case, "one source, mul = None", s1, None, 1.25, None, 0.0)


# ----------------------------------------------------------------------------- 5. B = 9
@pytest.mark.parametrize("case", ["rec9", "short"])
def test_nine_clips(case):
    """B = 9: analysis takes the non-temporal-store instantiations (B >= 8, babe_cqt_band_analysis), the record gather one full
    group of 8 clips and a ragged group of one.  Every clip within the bars; synthesis, gather and spec_scale of clip b equal their
    B = 1 call bit for bit (analysis runs another instantiation at B = 1: held to the bar only)."""
    hip = hip_of(case)
    B = 9
    assert B >= 8 and B % 8 == 1 and (hip.rec is None) == (case in CSR_CASES)
    spec = cc.rand_spec(case, B, cc.seed_of(case, 41))
    for kind in cc.ANALYSIS_KINDS:
        err = cc.coef_band_err(run_analysis(hip, case, spec, kind), cc.ref_analysis(case, spec, kind))
        print(f"B=9 analysis {case} {kind}: worst band per clip {np.array2string(err.max(1), precision=2)}")
        assert bool((err < ANALYSIS_BAR).all()), (case, kind, np.argwhere(~(err < ANALYSIS_BAR))[:8], cc.worst(err))
    co = cc.rand_coefs(case, B, cc.seed_of(case, 42))
    for kind in cc.SYNTHESIS_KINDS:
        got = run_synthesis(hip, case, co, kind)
        err = cc.bs_band_err(case, got, cc.ref_synthesis(case, co, kind))
        print(f"B=9 synthesis {case} {kind}: worst band per clip {np.array2string(err.max(1), precision=2)}")
        assert bool((err < SYNTHESIS_BAR).all()), (case, kind, cc.worst(err))
        for b in range(B):
            one = run_synthesis(hip, case, [c[b:b + 1] for c in co], kind)
            assert torch.equal(one[0], got[b]), f"{case} {kind}: clip {b} of B = 9 differs from its B = 1 call"
    seed, scale = cc.seed_of(case, 43), 2.0 / hip.Ls
    full = _gather_check(hip, case, B, seed, scale, True, hip.rec is not None)
    bs, mul = cc.rand_bs(case, B, seed), cc.rand_mul(case, seed + 1)
    for b in range(B):
        one = run_gather(hip, case, bs[b:b + 1], scale, mul, hip.rec is not None)
        assert torch.equal(one[0], full[b]), f"{case}: gather clip {b} of B = 9 differs from its B = 1 call"
    s2 = cc.rand_spec(case, B, cc.seed_of(case, 44))
    full = _spec_scale_check(hip, case, "two sources", spec, mul, 0.5, s2, 2.0)
    for b in range(B):
        one = run_spec_scale(hip, case, spec[b:b + 1], mul, 0.5, s2[b:b + 1], 2.0)
        assert torch.equal(one[0], full[b]), f"{case}: spec_scale clip {b} of B = 9 differs from its B = 1 call"


# ----------------------------------------------------------------------------- 6. BABE_CQT_ANALYTIC_WIN=0
def test_window_table_kernels_at_beta_1():
    """With the switch off the class has no polynomial: fwd's analysis and its adjoint read the Kaiser window from the table
    (the AN = false kernels) on a design whose default is the analytic form."""
    case = "short"
    hip = hip_of(case, analytic="0")
    assert hip.kaiser is None and hip_of(case).kaiser is not None
    spec = cc.rand_spec(case, 2, cc.seed_of(case, 51))
    err = cc.coef_band_err(run_analysis(hip, case, spec, "fwd"), cc.ref_analysis(case, spec, "fwd"))
    print(f"table-window analysis {case}: worst band {cc.worst(err):.2e}")
    assert bool((err < ANALYSIS_BAR).all()), (np.argwhere(~(err < ANALYSIS_BAR))[:8], cc.worst(err))
    co = cc.rand_coefs(case, 2, cc.seed_of(case, 52))
    got = run_synthesis(hip, case, co, "fwd_adjoint")
    err = cc.bs_band_err(case, got, cc.ref_synthesis(case, co, "fwd_adjoint"))
    print(f"table-window adjoint of analysis {case}: worst band {cc.worst(err):.2e}")
    assert bool((err < SYNTHESIS_BAR).all()), (np.argwhere(~(err < SYNTHESIS_BAR))[:8], cc.worst(err))


# ----------------------------------------------------------------------------- 7. whole transforms
@pytest.mark.parametrize("c_plan", ["1", "0"], ids=["plan", "class"])
@pytest.mark.parametrize("case", IDS)
def test_whole_transforms_vs_oracle(case, c_plan):
    """fwd / bwd / both adjoints / apply_hpf_DC against the float64 oracle (adjoints: float64 autograd through it), once through
    the library's plan (one C call per transform) and once with the class sequencing the kernels: coefficient outputs per band,
    time-domain outputs per clip, the bar of tests/test_gpu_cqt.py.  (Measured on a MI355X, largest over the cases, the same
    through the plan and through the class: fwd 3.97e-7, bwd 2.47e-7, fwd_adjoint 2.76e-7, bwd_adjoint 3.12e-7, hpf 2.30e-7,
    bwd(fwd(x)) 3.52e-7 - the bar has room to come down.)"""
    hip = hip_of(case, c_plan=c_plan)
    assert bool(hip._plan) == (c_plan == "1"), "the library's plan must exist for every case (and must not under BABE_CQT_C=0)"
    L, B, bar = cc.CASES[case]["L"], 2, cc.WHOLE_BAR
    g = torch.Generator().manual_seed(cc.seed_of(case, 61))
    x = 0.1 * torch.randn(B, L, generator=g)
    gx = torch.randn(B, L, generator=g)
    co = cc.rand_coefs(case, B, cc.seed_of(case, 62))
    dev = lambda ts: [t.cuda() for t in ts]
    res = {}
    fw = hip.fwd_planar(x.cuda())
    assert [tuple(c.shape) for c in fw] == [(B, 2, cc.CASES[case]["binsoct"], T) for T in cc.CASES[case]["T_oct"]]
    res["fwd (band)"] = cc.coef_band_err(fw, cc.oracle_fwd(case, x))
    res["bwd (clip)"] = cc.clip_err(hip.bwd_planar(dev(co)), cc.oracle_bwd(case, co))
    res["fwd_adjoint (clip)"] = cc.clip_err(hip.fwd_adjoint(dev(co)), cc.oracle_fwd_adjoint(case, co))
    res["bwd_adjoint (band)"] = cc.coef_band_err(hip.bwd_adjoint(gx.cuda()), cc.oracle_bwd_adjoint(case, gx))
    hp = cc.oracle(case).apply_hpf_DC(x.double())
    res["hpf (clip)"] = cc.clip_err(hip.apply_hpf_DC(x.cuda()), hp)
    cut = L - L // 3
    res["hpf, zero-padded input (clip)"] = cc.clip_err(hip.apply_hpf_DC(x[:, :cut].cuda()), cc.oracle(case).apply_hpf_DC(x[:, :cut].double()))
    res["bwd(fwd(x)) vs hpf (clip)"] = cc.clip_err(hip.bwd_planar(fw), hp)
    torch.cuda.synchronize()
    print(f"whole {case} {'plan' if c_plan == '1' else 'class'}: " + "  ".join(f"{k} {cc.worst(v):.2e}" for k, v in res.items()))
    for k, v in res.items():
        assert bool((v < bar).all()), (case, c_plan, k, cc.worst(v))


# ----------------------------------------------------------------------------- 8. refusals (host only: nothing is launched)
@pytest.mark.parametrize("name,args", [("binsoct = 1", (float(cc.FS), 2048, 6, 1, 1.0)),
                                       ("a band longer than 4096", (float(cc.FS), 32768, 8, 4, 1.0))])
def test_design_refusals(name, args):
    """babe_cqt_design_create is host code (no GPU call): both designs return NULL with the message set."""
    from babe_amd._lib import lib
    d = lib().babe_cqt_design_create(*args)
    if d:
        lib().babe_cqt_design_destroy(d)
    assert not d, name
    msg = lib().babe_last_error()
    assert msg.startswith(b"cqt design:") and (b"binsoct = %d" % args[3]) in msg, msg
    if name.startswith("a band"):
        assert b"4096" in msg, msg


def test_band_table_with_96_bands_per_workgroup_is_refused_before_any_launch():
    """check_bands() runs first in babe_cqt_band_analysis / _synthesis: -1 (BABE_ERR_ARG), "wg_count" in the message, the
    pre-filled outputs keep every value."""
    from babe_amd._lib import lib, stream
    case = "tiny"
    hip = hip_of(case)
    out = cc.GuardedCoefs(case, 1)
    for gd in out.bufs:
        gd.mid.fill_(7.0)
    s = hip._bands(out.views)
    s.max_wg_count = 96
    spec = cc.rand_spec(case, 1, 3, nan_above=False).cuda()
    rc = lib().babe_cqt_band_analysis(C.byref(s), spec.data_ptr(), hip.win_bwd_adj.data_ptr(), 1, stream())
    assert rc == -1 and b"wg_count" in lib().babe_last_error(), (rc, lib().babe_last_error())
    bs = cc.Guarded(hip.nwin * 2, fill=7.0, canary=-3.0)
    rc = lib().babe_cqt_band_synthesis(C.byref(s), bs.mid.data_ptr(), hip.win_bwd.data_ptr(), hip.nwin, 1, stream())
    assert rc == -1 and b"wg_count" in lib().babe_last_error(), (rc, lib().babe_last_error())
    torch.cuda.synchronize()
    assert all(bool((gd.mid == 7.0).all()) for gd in out.bufs) and bool((bs.mid == 7.0).all()), "refused, yet an output changed"
    assert out.canaries_intact() and bs.canaries_intact()
