"""The float64 statement of the log-spectral distance (tests/metrics_cases.py) against exact cases and against an independent
route, scipy.signal.stft; the band-to-bin rule of babe_amd.metrics; and the host-side refusals of babe_lsd_frames, which
launch nothing and so need no GPU."""
import numpy as np
import pytest

from tests import metrics_cases as MC


def test_scaled_copy_gives_twice_the_log_of_the_scale_in_every_frame():
    rng = np.random.RandomState(0)
    ref = 0.1 * rng.randn(2, 1500)
    assert MC.none_floored(ref, 256, 64)
    for c in (0.1, 3.0, 1e-2):
        est = c * ref
        assert MC.none_floored(est, 256, 64)
        for k_lo, k_hi in MC.bin_ranges(256):
            clip, fr = MC.lsd64(ref, est, 256, 64, k_lo, k_hi)
            assert fr.shape == (2, MC.num_frames(1500, 256, 64))
            assert np.abs(fr - 2 * abs(np.log10(c))).max() < 1e-12 and np.abs(clip - 2 * abs(np.log10(c))).max() < 1e-12


def test_silent_estimate_is_floored_in_every_bin():
    rng = np.random.RandomState(1)
    ref = 0.1 * rng.randn(1, 1000)
    fr = MC.frame_lsd64(ref, np.zeros_like(ref), 256, 100)
    pr = np.maximum(MC.powers64(ref, 256, 100), MC.FLOOR)
    assert np.abs(fr - np.sqrt((np.log10(pr / MC.FLOOR) ** 2).mean(-1))).max() < 1e-12
    # a reference below the floor as well: both sides floored, distance 0
    assert MC.frame_lsd64(1e-9 * ref, np.zeros_like(ref), 256, 100).max() == 0.0


@pytest.mark.parametrize("nfft,hop", [(256, 64), (256, 100), (512, 1), (256, 256)])
def test_frame_count(nfft, hop):
    x = np.random.RandomState(2).randn(1, nfft + 2 * hop + 3)
    for L, T in ((nfft, 1), (nfft + hop - 1, 1), (nfft + hop, 2)):
        assert MC.num_frames(L, nfft, hop) == T
        P = MC.powers64(x[:, :L], nfft, hop)
        assert P.shape == (1, T, nfft // 2 + 1)
        # the last frame starts at (T - 1) hop and the samples behind it are not used
        last = np.abs(np.fft.rfft(x[0, (T - 1) * hop:(T - 1) * hop + nfft] * MC.hann64(nfft))) ** 2
        assert np.allclose(P[0, -1], last, rtol=1e-12, atol=0)
    assert np.array_equal(MC.powers64(x[:, :nfft + hop - 1], nfft, hop), MC.powers64(x[:, :nfft], nfft, hop))


def test_window_is_the_periodic_hann():
    import torch
    for n in (256, 4096):
        assert np.abs(MC.hann64(n) - torch.hann_window(n, dtype=torch.float64).numpy()).max() < 1e-15


def test_band_to_bin_rule_at_its_edges():
    from babe_amd.metrics import band_bins, split_bin
    fs, nfft = 8000, 256                                          # bins 31.25 Hz apart
    assert band_bins(None, None, nfft) == (0, 129)
    for band, want in (((1000, 2000), (32, 65)),                  # both edges on a bin: both included
                       ((1000.1, 1999.9), (33, 64)), ((999.9, 2000.1), (32, 65)), ((0, 0), (0, 1)), ((0, 31.24), (0, 1)),
                       ((0, 31.25), (0, 2)), ((4000, 4000), (128, 129)), ((3990, 1e6), (128, 129)), ((0, 4000), (0, 129))):
        assert band_bins(band, fs, nfft) == want, band
        if all(float(f).is_integer() for f in band):
            assert MC.band_bins64(band, fs, nfft) == want, band
    fs, nfft = 44100, 2048                                        # a bin frequency computed in floating point, from either side
    for k in (1, 3, 7, 100, 333, 1023):
        f = k * fs / nfft
        assert band_bins((f, f), fs, nfft) == (k, k + 1)
        assert band_bins((np.nextafter(f, 0), np.nextafter(f, 1e9)), fs, nfft) == (k, k + 1)
        assert split_bin(f, fs, nfft) == k
    for bad in ((10, 20), (2000, 1000), (-1, 100), (4001, 5000)):
        with pytest.raises(ValueError):
            band_bins(bad, 8000, 256)
    with pytest.raises(ValueError):
        band_bins((100, 200), None, 256)
    assert split_bin(1000, 8000, 256) == 32 and split_bin(1000.1, 8000, 256) == 33
    for fc in (0, 4000.1):
        with pytest.raises(ValueError):
            split_bin(fc, 8000, 256)


@pytest.mark.parametrize("nfft,hop", [(256, 64), (512, 100), (2048, 512), (1024, 1024)])
def test_against_scipy_stft(nfft, hop):
    """An independent route to the same number: scipy's STFT with its own framing, window and scaling (the ratio of two powers
    is free of the scaling).  Inputs where no bin is floored; agreement to 1e-9."""
    from scipy.signal import stft
    ref, est = MC.signals(2, nfft + 7 * hop + 11, seed=nfft)
    ref, est = ref.astype(np.float64), est.astype(np.float64)
    assert MC.none_floored(ref, nfft, hop) and MC.none_floored(est, nfft, hop)
    kw = dict(window="hann", nperseg=nfft, noverlap=nfft - hop, boundary=None, padded=False)
    Zr, Ze = stft(ref, **kw)[2], stft(est, **kw)[2]              # [B, bins, T]
    assert Zr.shape == (2, nfft // 2 + 1, MC.num_frames(ref.shape[1], nfft, hop))
    d = np.log10(np.abs(Zr) ** 2) - np.log10(np.abs(Ze) ** 2)
    for k_lo, k_hi in MC.bin_ranges(nfft):
        want = np.sqrt((d[:, k_lo:k_hi] ** 2).mean(1))           # [B, T]
        clip, fr = MC.lsd64(ref, est, nfft, hop, k_lo, k_hi)
        assert np.abs(fr - want).max() < 1e-9 and np.abs(clip - want.mean(-1)).max() < 1e-9


def test_summary_statistics_helper():
    lines = [{"name": "a", "lsd": 1.0, "lsd_hf": 2.0, "segments": 2, "filter_db_mse": [1.0], "filter_db_mse_mean": 1.0},
             {"name": "b", "lsd": 3.0, "lsd_hf": 4.0, "segments": 4}]
    s = MC.summary_stats(lines)
    assert s == {"n": 2, "lsd": {"mean": 2.0, "std": 1.0}, "lsd_hf": {"mean": 3.0, "std": 1.0},
                 "filter_db_mse_mean": {"mean": 1.0, "std": 0.0}}


def test_library_refuses_bad_arguments_without_a_gpu():
    """babe_lsd_num_frames is host code, and babe_lsd_frames checks every argument before it launches: no pointer is followed."""
    import __graft_entry__ as ge
    ge.build()
    from babe_amd._lib import lib
    L = lib()
    assert L.babe_lsd_num_frames(256, 256, 64) == 1 and L.babe_lsd_num_frames(319, 256, 64) == 1
    assert L.babe_lsd_num_frames(320, 256, 64) == 2 and L.babe_lsd_num_frames(368368, 2048, 512) == 716
    for nfft in (256, 512, 1024, 2048, 4096):
        assert L.babe_lsd_num_frames(nfft, nfft, nfft) == 1
    for args in ((255, 256, 64), (600, 128, 64), (600, 8192, 64), (600, 300, 64), (600, 256, 0), (600, 256, 257)):
        assert L.babe_lsd_num_frames(*args) == -1, args
    FAKE = 0x1000
    call = lambda **k: L.babe_lsd_frames(*[dict(dict(r=FAKE, rb=600, e=FAKE, eb=600, L=600, B=1, nfft=256, hop=64, lo=0, hi=129,
                                                          fl=1e-10, fr=FAKE, cl=None), **k)[n]
                                            for n in ("r", "rb", "e", "eb", "L", "B", "nfft", "hop", "lo", "hi", "fl", "fr", "cl")], None)
    for k in (dict(nfft=100), dict(hop=0), dict(hop=300), dict(L=100), dict(lo=-1), dict(lo=129), dict(hi=130), dict(lo=9, hi=9),
              dict(fl=0.0), dict(fl=float("nan")), dict(B=0), dict(r=None), dict(e=None), dict(fr=None)):
        assert call(**k) == -1, k
        assert b"lsd_frames" in L.babe_last_error(), k
