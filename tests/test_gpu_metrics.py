"""Log-spectral distance on the GPU: babe_lsd_frames (csrc/metrics.hip) frame by frame and clip by clip against the float64
statement of tests/metrics_cases.py on the same fp32 inputs, and the Python surface babe_amd.metrics.  Needs a MI355X.

Every input is a view cut out of a NaN-filled buffer (NaN in front of the first row, between the rows and behind the last), so
a read outside [0, L) of a row turns the result into NaN; every output is cut out of a NaN-filled buffer, so a stray write shows.

Bar: metrics_cases.BAR = 2e-5 absolute on every frame value and every clip value - five times the 3.7e-6 by which a float32
restatement of the same algorithm on the CPU (packed complex64 FFT, fp32 log10) differs from the float64 statement on these
input families, for the GPU's log10f and its different butterfly and summation order.  Every case prints its largest error.

Measured on a MI355X.  A first, float32 version of the kernel (fft_lds_inplace, float32 window) missed the bar in four cases:
3.5e-5 on a frame over all bins at nfft 512, and 5.3e-5 / 3.2e-5 / 3.2e-4 on the Nyquist bin alone at nfft 1024 / 2048 / 4096;
the kernel now transforms in double, and the largest error over all 43 comparisons of this file is 1.03e-6 on a frame and
9.6e-7 on a clip ("Evaluation: log-spectral distance")."""
import functools

import numpy as np
import pytest
import torch

from tests import metrics_cases as MC

pytestmark = pytest.mark.gpu
ERR_ARG = -1


def framed(x, pad, off=0):
    """x [B, L] float32 numpy -> a [B, L] device view with row stride L + pad, starting 32 + off floats into a NaN-filled
    buffer whose allocation is 16-byte aligned (off = 1 puts every row of an L + pad = 0 mod 4 layout off that alignment)."""
    B, L = x.shape
    bs = L + pad
    buf = torch.full((64 + off + B * bs,), float("nan"), device="cuda")
    assert buf.data_ptr() % 16 == 0
    v = buf[32 + off:32 + off + B * bs].view(B, bs)[:, :L]
    v.copy_(torch.from_numpy(np.array(x)))               # (a copy: the cached cases are read-only)
    return v


def run(ref, est, nfft, hop, k_lo, k_hi, floor=MC.FLOOR, want_clip=True):
    """One babe_lsd_frames call on device views; returns (frames [B,T], clip [B] or None) after checking the guard bands."""
    from babe_amd._lib import check, lib, ptr, stream
    B, L = ref.shape
    T = lib().babe_lsd_num_frames(L, nfft, hop)
    assert T == MC.num_frames(L, nfft, hop)
    fbuf = torch.full((B * T + 16,), float("nan"), device="cuda")
    cbuf = torch.full((B + 16,), float("nan"), device="cuda")
    fr, cl = fbuf[8:8 + B * T].view(B, T), cbuf[8:8 + B]
    check(lib().babe_lsd_frames(ptr(ref), ref.stride(0), ptr(est), est.stride(0), L, B, nfft, hop, k_lo, k_hi, floor, ptr(fr),
                                ptr(cl) if want_clip else None, stream()), "lsd_frames")
    torch.cuda.synchronize()
    assert bool(torch.isnan(fbuf[:8]).all()) and bool(torch.isnan(fbuf[8 + B * T:]).all())
    assert bool(torch.isnan(cbuf[:8]).all()) and bool(torch.isnan(cbuf[8 + B:]).all())
    if not want_clip:
        assert bool(torch.isnan(cbuf).all())
    return fr.clone(), (cl.clone() if want_clip else None)


def compare(tag, fr, cl, want_fr):
    """Largest frame and clip error against the float64 frame values want_fr [B,T]; prints, then holds both to the bar."""
    got = fr.double().cpu().numpy()
    assert np.isfinite(got).all(), tag
    ef = float(np.abs(got - want_fr).max())
    ec = float(np.abs(cl.double().cpu().numpy() - want_fr.mean(-1)).max()) if cl is not None else 0.0
    print(f"{tag}: max frame error {ef:.3e}, max clip error {ec:.3e} (bar {MC.BAR:.0e})")
    assert ef <= MC.BAR and ec <= MC.BAR, (tag, ef, ec)
    return max(ef, ec)


@functools.lru_cache(maxsize=None)
def case(nfft, hop, L, B=2):
    """(ref, est) float32 numpy of one geometry, made once; no bin of either is floored."""
    ref, est = MC.signals(B, L, seed=nfft + hop + L)
    assert MC.none_floored(ref, nfft, hop) and MC.none_floored(est, nfft, hop)
    ref.setflags(write=False)
    est.setflags(write=False)
    return ref, est


@pytest.mark.parametrize("nfft", MC.NFFTS)
def test_every_transform_size_and_bin_range(nfft):
    """Both log2 paths of fft_lds_inplace; all bins, DC, bin 1, Nyquist and [nfft/8, Nyquist] at each size."""
    hop, L = nfft // 4, nfft + 3 * (nfft // 4) + 5
    ref, est = case(nfft, hop, L)
    r, e = framed(ref, 3), framed(est, 6)
    for k_lo, k_hi in MC.bin_ranges(nfft):
        fr, cl = run(r, e, nfft, hop, k_lo, k_hi)
        compare(f"nfft {nfft} bins [{k_lo},{k_hi})", fr, cl, MC.frame_lsd64(ref, est, nfft, hop, k_lo, k_hi))


@pytest.mark.parametrize("nfft,hop,L,what", MC.GEOMETRY_CASES, ids=[c[3] for c in MC.GEOMETRY_CASES])
def test_frame_geometry(nfft, hop, L, what):
    ref, est = case(nfft, hop, L)
    r, e = framed(ref, 3), framed(est, 6)
    for k_lo, k_hi in ((0, nfft // 2 + 1), (nfft // 8, nfft // 2 + 1)):
        fr, cl = run(r, e, nfft, hop, k_lo, k_hi)
        assert fr.shape[1] == MC.num_frames(L, nfft, hop)
        compare(f"{what} bins [{k_lo},{k_hi})", fr, cl, MC.frame_lsd64(ref, est, nfft, hop, k_lo, k_hi))


def test_strides_and_alignment():
    """B = 3, ref_bs != est_bs != L, the estimate's rows one float off 16-byte alignment."""
    nfft, hop, L = 256, 64, 256 + 3 * 64 + 5
    ref, est = case(nfft, hop, L, 3)
    r, e = framed(ref, 7), framed(est, 3, off=1)               # strides 460 and 456
    assert r.stride(0) != e.stride(0) and L not in (r.stride(0), e.stride(0))
    assert r.data_ptr() % 16 == 0 and e.data_ptr() % 16 == 4 and e.stride(0) % 4 == 0
    fr, cl = run(r, e, nfft, hop, 0, nfft // 2 + 1)
    compare("B 3, strides 460 / 456, est off by one float", fr, cl, MC.frame_lsd64(ref, est, nfft, hop))


def test_clip_output_may_be_null_and_two_calls_agree_bit_for_bit():
    nfft, hop, L = 256, 64, 256 + 3 * 64 + 5
    ref, est = case(nfft, hop, L)
    r, e = framed(ref, 3), framed(est, 6)
    fr0, cl0 = run(r, e, nfft, hop, 0, nfft // 2 + 1)
    fr1, none = run(r, e, nfft, hop, 0, nfft // 2 + 1, want_clip=False)
    fr2, cl2 = run(r, e, nfft, hop, 0, nfft // 2 + 1)
    assert none is None and torch.equal(fr0, fr1) and torch.equal(fr0, fr2) and torch.equal(cl0, cl2)
    nfft, hop, L = 2048, 512, 2048 + 299 * 512                  # 300 frames: the clip mean's threads take two frames each
    ref, est = MC.signals(1, L, seed=5)                          # (only compared with itself: a floored bin would not matter)
    r, e = framed(ref, 3), framed(est, 6)
    a, b = run(r, e, nfft, hop, 0, nfft // 2 + 1), run(r, e, nfft, hop, 0, nfft // 2 + 1)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("nfft", (256, 2048))
def test_exact_cases(nfft):
    """est = 0.1f ref: 2.0 in every frame.  est = ref: at most the bar (not exactly 0: the two spectra leave the packed FFT
    through different arithmetic).  est = 0: every est bin is floored, against float64."""
    hop, L = nfft // 4, nfft + 3 * (nfft // 4) + 5
    ref, _ = case(nfft, hop, L)
    r = framed(ref, 3)
    scaled = (np.float32(0.1) * ref).astype(np.float32)
    fr, cl = run(r, framed(scaled, 6), nfft, hop, 0, nfft // 2 + 1)
    assert MC.none_floored(scaled, nfft, hop)
    compare(f"nfft {nfft} est = 0.1 ref", fr, cl, np.full(tuple(fr.shape), 2.0))
    fr, cl = run(r, framed(ref.copy(), 6), nfft, hop, 0, nfft // 2 + 1)
    compare(f"nfft {nfft} est = ref", fr, cl, np.zeros(tuple(fr.shape)))
    zero = np.zeros_like(ref)
    want = MC.frame_lsd64(ref, zero, nfft, hop)
    pr = np.maximum(MC.powers64(ref, nfft, hop), MC.FLOOR)
    assert np.allclose(want, np.sqrt((np.log10(pr / MC.FLOOR) ** 2).mean(-1)), rtol=0, atol=1e-12)
    fr, cl = run(r, framed(zero, 6), nfft, hop, 0, nfft // 2 + 1)
    compare(f"nfft {nfft} est = 0", fr, cl, want)


def test_refusals_launch_nothing():
    from babe_amd._lib import lib, ptr, stream
    Lb = lib()
    L, nfft, hop = 600, 256, 64
    x = torch.ones(2, L, device="cuda")
    fr = torch.full((2, 6), 7.0, device="cuda")                  # T = 1 + (600 - 256) // 64 = 6
    cl = torch.full((2,), 7.0, device="cuda")
    good = dict(ref=ptr(x), ref_bs=L, est=ptr(x), est_bs=L, L=L, B=2, nfft=nfft, hop=hop, k_lo=0, k_hi=129, floor=1e-10,
                fr=ptr(fr), cl=ptr(cl))
    order = ("ref", "ref_bs", "est", "est_bs", "L", "B", "nfft", "hop", "k_lo", "k_hi", "floor", "fr", "cl")
    bad = [dict(nfft=128), dict(nfft=8192), dict(nfft=300), dict(nfft=0), dict(hop=0), dict(hop=257), dict(hop=-1), dict(L=255),
           dict(L=0), dict(k_lo=-1), dict(k_lo=129, k_hi=129), dict(k_lo=5, k_hi=5), dict(k_lo=6, k_hi=5), dict(k_hi=130),
           dict(floor=0.0), dict(floor=-1.0), dict(floor=float("nan")), dict(B=0), dict(B=-2), dict(ref=None), dict(est=None),
           dict(fr=None)]
    for change in bad:
        a = dict(good, **change)
        assert Lb.babe_lsd_frames(*[a[k] for k in order], stream()) == ERR_ARG, change
        assert b"lsd_frames" in Lb.babe_last_error(), change
    torch.cuda.synchronize()
    assert bool((fr == 7.0).all()) and bool((cl == 7.0).all())
    assert Lb.babe_lsd_frames(*[good[k] for k in order], stream()) == 0          # the unchanged call is accepted
    torch.cuda.synchronize()
    assert bool((fr != 7.0).all()) and bool((cl != 7.0).all()) and bool(torch.isfinite(fr).all())      # ... and writes both
    for args in ((255, 256, 64), (600, 128, 64), (600, 256, 0), (600, 256, 257), (600, 300, 64)):
        assert Lb.babe_lsd_num_frames(*args) == -1
    assert Lb.babe_lsd_num_frames(256, 256, 64) == 1 and Lb.babe_lsd_num_frames(319, 256, 64) == 1
    assert Lb.babe_lsd_num_frames(320, 256, 64) == 2


def test_python_surface():
    from babe_amd import metrics as M
    from babe_amd.stft import STFTOps
    nfft, hop, L, fs = 256, 64, 256 + 3 * 64 + 5, 8000
    ref, est = case(nfft, hop, L, 3)
    r, e = framed(ref, 7), framed(est, 3, off=1)
    clip, fr = M.lsd(r, e, nfft=nfft, hop=hop, per_frame=True)
    want = MC.frame_lsd64(ref, est, nfft, hop)
    assert clip.shape == (3,) and fr.shape == (3, want.shape[1])
    compare("metrics.lsd", fr, clip, want)
    assert torch.equal(M.lsd(r, e, nfft=nfft, hop=hop), clip)
    one = M.lsd(r[1], e[1], nfft=nfft, hop=hop)                  # [L] -> [1]
    assert one.shape == (1,) and torch.equal(one, clip[1:2])
    # a band in Hz: bins ceil(1000 * 256 / 8000) = 32 .. floor(2010 * 256 / 8000) = 64, both included
    assert M.band_bins((1000, 2010), fs, nfft) == MC.band_bins64((1000, 2010), fs, nfft) == (32, 65)
    b = M.lsd(r, e, nfft=nfft, hop=hop, fs=fs, band=(1000, 2010))
    assert np.abs(b.double().cpu().numpy() - MC.frame_lsd64(ref, est, nfft, hop, 32, 65).mean(-1)).max() <= MC.BAR
    assert M.band_bins((0, 1e9), fs, nfft) == (0, 129)           # f_hi beyond Nyquist stops at nfft / 2
    s = M.lsd_split(r, e, fs, 1000.0, nfft=nfft, hop=hop)
    assert set(s) == {"lsd", "lsd_lf", "lsd_hf"} and torch.equal(s["lsd"], clip)
    for key, (k_lo, k_hi) in (("lsd_lf", (0, 32)), ("lsd_hf", (32, 129))):
        assert np.abs(s[key].double().cpu().numpy() - MC.frame_lsd64(ref, est, nfft, hop, k_lo, k_hi).mean(-1)).max() <= MC.BAR
    assert bool((s["lsd_hf"] > s["lsd_lf"]).all())               # the estimate is a low-pass of the reference at 1000 Hz
    # errors
    for call in (lambda: M.lsd(r, e[:, :-1], nfft=nfft, hop=hop), lambda: M.lsd(r[:, ::2], e[:, ::2], nfft=nfft, hop=hop),
                 lambda: M.lsd(r, e, nfft=nfft, hop=hop, band=(100, 200)), lambda: M.lsd(r, e, nfft=nfft, hop=hop, fs=fs, band=(10, 20)),
                 lambda: M.lsd(r, e, nfft=nfft, hop=hop, fs=fs, band=(2000, 1000)), lambda: M.lsd(r, e, nfft=300, hop=hop),
                 lambda: M.lsd(r, e, nfft=1024, hop=hop), lambda: M.lsd(r.double(), e.double(), nfft=nfft, hop=hop),
                 lambda: M.lsd_split(r, e, fs, 0.0, nfft=nfft, hop=hop), lambda: M.lsd_split(r, e, fs, 4001.0, nfft=nfft, hop=hop)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(RuntimeError):
        M.lsd(torch.from_numpy(ref), torch.from_numpy(est), nfft=nfft, hop=hop)
    # filter_db_mse against float64 numpy on the H that STFTOps.design_filter returns
    tru = torch.tensor([[1000.0, 2000.0], [-20.0, -40.0]])
    ests = torch.tensor([[[900.0, 2100.0], [-18.0, -35.0]], [[1000.0, 2000.0], [-20.0, -40.0]], [[500.0, 600.0], [-5.0, -50.0]]])
    st = STFTOps(512, 512, 22050, "cuda")
    Ht, He = st.design_filter(tru.cuda()).double().cpu().numpy(), st.design_filter(ests.cuda()).double().cpu().numpy()
    want = ((20 * np.log10(Ht)[None] - 20 * np.log10(He)) ** 2).mean(-1)
    got = M.filter_db_mse(tru, ests.cuda(), 22050, 512)
    assert got.shape == (3,) and float(got[1]) == 0.0
    assert np.allclose(got.double().cpu().numpy(), want, rtol=1e-4, atol=1e-6), (got, want)
    assert M.filter_db_mse(tru, ests[0], 22050, 512).shape == (1,)
    with pytest.raises(ValueError):
        M.filter_db_mse(tru[0], ests, 22050, 512)
