"""Pre-emphasis filters of the training loss.  Mirrors the call surface of the reference's utils/training_utils.py FIRFilter
(:55-138, after auraloss.perceptual; Wright & Valimaki 2019): the filter design is host-side scipy exactly like the reference, the
filtering itself is the HIP FIR (babe_fir_same) instead of F.conv1d.  Device tensors only, no CPU fallback."""
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
