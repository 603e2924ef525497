"""Pre-emphasis filters of the training loss.  Mirrors the call surface of the reference's utils/training_utils.py FIRFilter
(:55-138, after auraloss.perceptual; Wright & Valimaki 2019): the filter design is host-side scipy exactly like the reference, the
filtering itself is the HIP FIR (babe_fir_same) instead of F.conv1d.  Device tensors only, no CPU fallback.
resample_batch (:140-221) is the trainer's batch resampler on the HIP sinc resampler."""
import numpy as np
import scipy.signal
import torch

from ..stft import fir_same


def aweighting_taps(fs, ntaps):
    """Linear-phase FIR fit of the A-weighting curve at sample rate fs (float64 [ntaps]): the analog prototype of IEC 61672 (four
    poles at 20.6 Hz and 12194 Hz in pairs, 107.7 Hz and 737.9 Hz, four zeros at DC, 0 dB at 1 kHz) through the bilinear transform,
    its magnitude on 512 frequencies, least-squares fitted (scipy.signal.firls)."""
    f1, f2, f3, f4, a1000 = 20.598997, 107.65265, 737.86223, 12194.217, 1.9997
    w1, w2, w3, w4 = (2 * np.pi * f for f in (f1, f2, f3, f4))
    num = [w4 ** 2 * 10 ** (a1000 / 20), 0, 0, 0, 0]
    den = np.polymul([1, 2 * w4, w4 ** 2], [1, 2 * w1, w1 ** 2])
    den = np.polymul(np.polymul(den, [1, w3]), [1, w2])
    b, a = scipy.signal.bilinear(num, den, fs=fs)
    w, h = scipy.signal.freqz(b, a, worN=512, fs=fs)
    return scipy.signal.firls(ntaps, w, abs(h), fs=fs)


def _rate_rule(fs, fs_target):
    """(orig, new) handed to the resampler for one source rate - the table of reference training_utils.py:140-221 - or None
    where the row passes through as it is."""
    fs, fs_target = int(fs), int(fs_target)
    if fs_target == 22050:
        rule = {44100: (2, 1), 48000: (160 * 2, 147)}
    elif fs_target == 44100:
        rule = {44100: None, 48000: (160, 147), 22050: (1, 2)}
    else:
        rule = {44100: (44100, fs_target), 48000: (48000, fs_target)}
    if fs not in rule:
        raise ValueError(f"resample_batch: no rule for a {fs} Hz row and target {fs_target} Hz (known: {sorted(rule)})")
    return rule[fs]


def resample_batch(audio, fs, fs_target, length_target):
    """audio [B,L] on the GPU, fs one rate per row (tensor or list) -> [B, length_target] at fs_target: the reference's rule
    table (utils/training_utils.py:140-221; 48000 -> 44100 is its approximation 160/147, 48000 -> 22050 is 320/147) on
    babe_amd.resample.resample, the HIP sinc resampler.  A batch at one rate is one launch; mixed rates go row by row.  The
    result is cropped to [..., :length_target].
    Two deliberate departures: a rate without a rule raises ValueError (the reference prints a warning and copies the row
    unresampled, i.e. trains on audio at the wrong pitch), and so does a resampled row shorter than length_target (the
    reference returns the short batch, or fails on the row assignment)."""
    from ..resample import resample
    rates = [int(r) for r in (fs.tolist() if torch.is_tensor(fs) else fs)]
    if audio.dim() != 2 or len(rates) != audio.shape[0]:
        raise ValueError(f"resample_batch: audio {tuple(audio.shape)} needs one rate per row, got {len(rates)}")
    rules = [_rate_rule(r, fs_target) for r in rates]

    def one(x, rule, what):
        y = x if rule is None else resample(x, rule[0], rule[1])
        if y.shape[-1] < length_target:
            raise ValueError(f"resample_batch: {what} gives {y.shape[-1]} samples at {fs_target} Hz, fewer than "
                             f"length_target = {length_target}")
        return y[..., :length_target]

    if len(set(rates)) == 1:
        return one(audio, rules[0], f"{audio.shape[-1]} samples at {rates[0]} Hz")
    out = torch.empty(audio.shape[0], length_target, device=audio.device, dtype=torch.float32)
    for i, rule in enumerate(rules):
        out[i] = one(audio[i], rule, f"row {i} ({audio.shape[-1]} samples at {rates[i]} Hz)")
    return out


class _Fir(torch.autograd.Function):
    @staticmethod
    def forward(ctx, error, taps):
        ctx.save_for_backward(taps)
        return fir_same(error, taps)

    @staticmethod
    def backward(ctx, g):
        taps, = ctx.saved_tensors
        return fir_same(g.contiguous(), taps, adjoint=True), None


class FIRFilter:
    """FIRFilter(filter_type, coef, fs, ntaps): "hp" first-order high-pass [1, -coef, 0], "fd" folded differentiator
    [1, 0, -coef], "aw" A-weighting with ntaps taps.  `taps` is a float32 tensor [K]; calling the filter on an error [B,L] returns
    out[n] = sum_k taps[k] * error[n + k - K//2] (zeros outside the signal; F.conv1d(padding=K//2), no tap flip), with the
    transposed FIR as its backward.  For "hp" / "fd" K is 3 whatever ntaps says (the reference pads those by ntaps//2 as well, which
    at its default ntaps = 101 returns L + 98 samples; the two agree at ntaps = 3)."""

    def __init__(self, filter_type="hp", coef=0.85, fs=44100, ntaps=101):
        self.filter_type, self.coef, self.fs, self.ntaps = filter_type, coef, fs, ntaps
        if ntaps % 2 == 0:
            raise ValueError(f"ntaps must be odd (ntaps={ntaps}).")
        if filter_type == "hp":
            self.taps = torch.tensor([1, -coef, 0], dtype=torch.float32)
        elif filter_type == "fd":
            self.taps = torch.tensor([1, 0, -coef], dtype=torch.float32)
        elif filter_type == "aw":
            self.taps = torch.tensor(aweighting_taps(fs, ntaps).astype("float32"))
        else:
            raise ValueError(f"filter_type={filter_type!r} (one of 'hp', 'fd', 'aw')")

    def to(self, device):
        """Move the taps (done lazily by the first call on a device tensor)."""
        if self.taps.device != torch.device(device):
            self.taps = self.taps.to(device)
        return self

    def __call__(self, error):
        if not error.is_cuda:
            raise RuntimeError("babe_amd.FIRFilter runs on the GPU only (no CPU fallback)")
        self.to(error.device)
        return _Fir.apply(error if error.stride(-1) == 1 else error.contiguous(), self.taps)

    forward = __call__
