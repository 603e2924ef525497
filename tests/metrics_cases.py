"""Float64 statement of the log-spectral distance (LSD) and the cases of its tests (tests/test_metrics_cases_cpu.py pins the
statement on the CPU, tests/test_gpu_metrics.py runs csrc/metrics.hip against it).  numpy only.

The definition (this project's own; INTEGRATION.md "Evaluating a prior"): frames of nfft samples every hop samples, full frames
only, T = 1 + (L - nfft) // hop, no centring, no padding; periodic Hann window w[i] = 0.5 - 0.5 cos(2 pi i / nfft);
P = |rfft(w frame)|^2, unnormalised, floored at `floor`; d[t,k] = log10 Pref - log10 Pest; lsd[t] = sqrt(mean over k in
[k_lo, k_hi) of d^2); LSD = mean over t of lsd[t].
"""
import numpy as np

FLOOR = 1e-10
BAR = 2e-5                 # absolute, on every frame value and every clip value (five times the 3.7e-6 by which a float32
#                            restatement of the packed-FFT algorithm on the CPU differs from this statement, nfft 256 .. 4096)
NFFTS = (256, 512, 1024, 2048, 4096)

# (nfft, hop, L, what the row reaches); nfft = 256, hop = 64 unless the row is about something else
GEOMETRY_CASES = [
    (256, 64, 256, "L = nfft: one frame"),
    (256, 64, 256 + 3 * 64 + 5, "four frames, the last 5 samples unused"),
    (512, 1, 512 + 8, "hop = 1: nine frames one sample apart"),
    (256, 256, 3 * 256, "hop = nfft: frames side by side"),
    (256, 100, 256 + 4 * 100 + 37, "a hop that does not divide nfft"),
]


def bin_ranges(nfft):
    """The bin ranges every transform size is run with: all bins, DC alone, bin 1 alone, Nyquist alone (DC and Nyquist are where
    the separation of two real signals out of one complex FFT differs), and the upper seven eighths."""
    h = nfft // 2
    return [(0, h + 1), (0, 1), (1, 2), (h, h + 1), (nfft // 8, h + 1)]


def num_frames(L, nfft, hop):
    return 1 + (L - nfft) // hop


def hann64(nfft):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(nfft, dtype=np.float64) / nfft)


def powers64(x, nfft, hop):
    """[B, L] -> unfloored P [B, T, nfft/2 + 1] in float64."""
    x = np.asarray(x, dtype=np.float64)
    x = x[None] if x.ndim == 1 else x
    T = num_frames(x.shape[-1], nfft, hop)
    idx = hop * np.arange(T)[:, None] + np.arange(nfft)[None, :]
    return np.abs(np.fft.rfft(x[:, idx] * hann64(nfft), axis=-1)) ** 2


def frame_lsd64(ref, est, nfft, hop, k_lo=0, k_hi=None, floor=FLOOR):
    """[B, L] x 2 -> lsd [B, T] in float64."""
    k_hi = nfft // 2 + 1 if k_hi is None else k_hi
    pr = np.maximum(powers64(ref, nfft, hop), floor)[..., k_lo:k_hi]
    pe = np.maximum(powers64(est, nfft, hop), floor)[..., k_lo:k_hi]
    d = np.log10(pr) - np.log10(pe)
    return np.sqrt((d * d).mean(-1))


def lsd64(ref, est, nfft, hop, k_lo=0, k_hi=None, floor=FLOOR):
    """-> (clip LSD [B], frame values [B, T])."""
    f = frame_lsd64(ref, est, nfft, hop, k_lo, k_hi, floor)
    return f.mean(-1), f


def band_bins64(band, fs, nfft):
    """(f_lo, f_hi) Hz -> [k_lo, k_hi): bins ceil(f_lo nfft / fs) .. min(floor(f_hi nfft / fs), nfft / 2), both included, in
    exact rational arithmetic on integer arguments."""
    f_lo, f_hi = band
    k_lo = -((-int(f_lo) * nfft) // int(fs))
    k_hi = min((int(f_hi) * nfft) // int(fs), nfft // 2)
    return k_lo, k_hi + 1


def signals(B, L, seed):
    """The test signals: ref = 0.1 randn, est = a 6th-order Butterworth low-pass of ref at a quarter of Nyquist plus 1e-3 randn,
    both float32 [B, L].  With floor = 1e-10 no bin of either is floored (the tests assert it on the float64 powers)."""
    from scipy.signal import butter, sosfilt
    rng = np.random.RandomState(seed)
    ref = 0.1 * rng.randn(B, L)
    est = sosfilt(butter(6, 0.25, output="sos"), ref, axis=-1) + 1e-3 * rng.randn(B, L)
    return ref.astype(np.float32), est.astype(np.float32)


def none_floored(x, nfft, hop, floor=FLOOR):
    return bool((powers64(x, nfft, hop) > floor).all())


def summary_stats(lines):
    """What summary.json must hold for these metrics.jsonl lines: n, and mean / std (population) of every metric - the keys that
    start with "lsd", and "filter_db_mse_mean"."""
    keys = sorted({k for ln in lines for k in ln if k.startswith("lsd") or k == "filter_db_mse_mean"})
    out = {"n": len(lines)}
    for k in keys:
        v = np.array([ln[k] for ln in lines if k in ln], dtype=np.float64)
        out[k] = {"mean": float(v.mean()), "std": float(v.std())}
    return out
