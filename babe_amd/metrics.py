"""Objective metrics of an evaluation run on the babe_hip kernels: log-spectral distance (LSD, csrc/metrics.hip) and the dB error
of an estimated low-pass filter.  GPU only, like the rest of the package.

LSD is this project's own definition - the reference computes none ("Evaluating a prior"): frames of nfft
samples every hop samples, full frames only (T = 1 + (L - nfft) // hop; no centring, no padding, the samples behind the last
full frame are not used), periodic Hann window, P = |rfft(w frame)|^2 floored at `floor`, d = log10 Pref - log10 Pest,
lsd[t] = sqrt(mean_k d^2) over the selected bins, LSD = mean_t lsd[t]."""
import math

import torch

from ._lib import check, lib, ptr, stream


def _bin_pos(f, fs, nfft):
    """f in bins, f nfft / fs; a value within 1e-9 of an integer IS that integer (a bin frequency k fs / nfft computed in floating
    point must select bin k from either side)."""
    x = float(f) * nfft / float(fs)
    r = round(x)
    return float(r) if abs(x - r) <= 1e-9 * max(1.0, abs(x)) else x


def band_bins(band, fs, nfft):
    """band = (f_lo, f_hi) in Hz -> (k_lo, k_hi): the bins ceil(f_lo nfft / fs) .. min(floor(f_hi nfft / fs), nfft / 2), both
    included, as the half-open range [k_lo, k_hi).  None: every bin."""
    if band is None:
        return 0, nfft // 2 + 1
    if fs is None:
        raise ValueError("lsd: band=(f_lo, f_hi) is in Hz and needs fs")
    f_lo, f_hi = band
    if not (0 <= f_lo <= f_hi):
        raise ValueError(f"lsd: band {band!r} must satisfy 0 <= f_lo <= f_hi")
    k_lo = int(math.ceil(_bin_pos(f_lo, fs, nfft)))
    k_hi = min(int(math.floor(_bin_pos(f_hi, fs, nfft))), nfft // 2) + 1
    if k_lo >= k_hi:
        raise ValueError(f"lsd: band {band!r} Hz holds no bin of nfft = {nfft} at fs = {fs}")
    return k_lo, k_hi


def split_bin(fc, fs, nfft):
    """First bin at or above fc: bins [0, ks) lie below fc, bins [ks, nfft / 2] from fc to Nyquist."""
    ks = int(math.ceil(_bin_pos(fc, fs, nfft)))
    if not (0 < ks <= nfft // 2):
        raise ValueError(f"lsd_split: fc = {fc} Hz leaves one side without a bin (nfft = {nfft}, fs = {fs})")
    return ks


def _lsd_bins(ref, est, nfft, hop, k_lo, k_hi, floor, per_frame):
    if not (isinstance(ref, torch.Tensor) and isinstance(est, torch.Tensor) and ref.is_cuda and est.is_cuda):
        raise RuntimeError("babe_amd.metrics.lsd runs on the GPU only (no CPU fallback)")
    if ref.dtype != torch.float32 or est.dtype != torch.float32 or ref.shape != est.shape or ref.dim() not in (1, 2):
        raise ValueError(f"lsd: ref and est must be float32 [B,L] or [L] tensors of one shape (got {tuple(ref.shape)} {ref.dtype}, "
                         f"{tuple(est.shape)} {est.dtype})")
    r, e = (ref.unsqueeze(0), est.unsqueeze(0)) if ref.dim() == 1 else (ref, est)
    B, L = r.shape
    if B < 1 or r.stride(1) != 1 or e.stride(1) != 1:
        raise ValueError("lsd: ref and est need at least one row, and rows of contiguous samples")
    T = lib().babe_lsd_num_frames(L, int(nfft), int(hop))
    if T < 1:
        raise ValueError(f"lsd: nfft = {nfft} (a power of two, 256 .. 4096), hop = {hop} (1 .. nfft) and L = {L} (>= nfft) give no frame")
    if not (0 <= k_lo < k_hi <= nfft // 2 + 1) or not floor > 0:
        raise ValueError(f"lsd: bins [{k_lo}, {k_hi}) of {nfft // 2 + 1}, floor = {floor}")
    frames = torch.empty(B, T, device=r.device)
    clip = torch.empty(B, device=r.device)
    check(lib().babe_lsd_frames(ptr(r), r.stride(0) if B > 1 else L, ptr(e), e.stride(0) if B > 1 else L, L, B, int(nfft), int(hop),
                                k_lo, k_hi, float(floor), ptr(frames), ptr(clip), stream(r)), "lsd_frames")
    return (clip, frames) if per_frame else clip


def lsd(ref, est, *, nfft=2048, hop=512, fs=None, band=None, floor=1e-10, per_frame=False):
    """Log-spectral distance of `est` against `ref`: [B,L] or [L] CUDA float32 tensors of equal shape with contiguous rows (the
    rows of the two may have different strides) -> [B], or ([B], [B,T] per-frame values) with per_frame.  band=(f_lo, f_hi) in Hz
    (needs fs) restricts the mean over bins to ceil(f_lo nfft / fs) .. min(floor(f_hi nfft / fs), nfft / 2), both included.
    ValueError for a bad shape, stride or band; RuntimeError for CPU tensors.  One kernel launch plus the mean over frames; two calls
    agree bit for bit."""
    k_lo, k_hi = band_bins(band, fs, int(nfft))
    return _lsd_bins(ref, est, int(nfft), int(hop), k_lo, k_hi, floor, per_frame)


def lsd_split(ref, est, fs, fc, *, nfft=2048, hop=512, floor=1e-10):
    """dict(lsd=, lsd_lf=, lsd_hf=), each [B]: over every bin, over the bins below fc and over the bins from fc to Nyquist (three
    kernel calls)."""
    nfft = int(nfft)
    ks = split_bin(fc, fs, nfft)
    return dict(lsd=_lsd_bins(ref, est, nfft, hop, 0, nfft // 2 + 1, floor, False),
                lsd_lf=_lsd_bins(ref, est, nfft, hop, 0, ks, floor, False),
                lsd_hf=_lsd_bins(ref, est, nfft, hop, ks, nfft // 2 + 1, floor, False))


def filter_db_mse(fp_true, fp_est, fs, nfft):
    """mean_k (20 log10 H_true[k] - 20 log10 H_est[k])^2 over the nfft / 2 + 1 bins, both H designed by babe_design_filter
    (STFTOps.design_filter) from breakpoints [2,K] or [P,2,K] (a [2,K] side is shared by all P of the other) -> [P].  The number
    the reference's tester reports for a blind run (testing/blind_bwe_tester_small.py:398-404)."""
    from .stft import STFTOps
    a, b = torch.as_tensor(fp_true, dtype=torch.float32), torch.as_tensor(fp_est, dtype=torch.float32)
    # (the breakpoints are a handful of numbers and may come from a configuration or a pickle: they are moved to the GPU, where
    # both filters are designed; the current device if neither lives on one)
    dev = a.device if a.is_cuda else b.device if b.is_cuda else torch.device("cuda", torch.cuda.current_device())
    for p in (a, b):
        if p.dim() not in (2, 3) or p.shape[-2] != 2:
            raise ValueError(f"filter_db_mse: filter parameters must be [2,K] or [P,2,K] (got {tuple(p.shape)})")
    a3, b3 = (a.unsqueeze(0) if a.dim() == 2 else a).to(dev), (b.unsqueeze(0) if b.dim() == 2 else b).to(dev)
    if a3.shape[0] != b3.shape[0] and 1 not in (a3.shape[0], b3.shape[0]):
        raise ValueError(f"filter_db_mse: {a3.shape[0]} true and {b3.shape[0]} estimated parameter sets")
    st = STFTOps(int(nfft), int(nfft), float(fs), dev)
    Ha, Hb = st.design_filter(a3), st.design_filter(b3)
    return ((20.0 * torch.log10(Ha) - 20.0 * torch.log10(Hb)) ** 2).mean(-1)              # ([1,nbins] broadcasts against [P,nbins])
