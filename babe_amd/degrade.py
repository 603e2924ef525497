"""Known degradations of BlindSampler.predict_bwe beyond the FIR - the reference's 'cheby1' (torchaudio.functional.lfilter,
clamp=False), 'biquad' (torchaudio.functional.biquad: lfilter with its default clamp=True), 'resample'
(torchaudio.functional.resample(x, int(100 factor), 100)) and 'decimate' (x[..., 0:-1:factor]),
testing/blind_bwe_sampler.py:219-230 - each as a forward A and its adjoint A^T on the HIP kernels of csrc/degrade.hip.

Coefficients are prepared on the host the way lfilter sees them: rounded to float32 (`torch.Tensor(b)`), divided by a[0] in
float32.  The recursion itself runs in float64 on the GPU.  Device tensors only, no CPU fallback."""
import numpy as np
import torch

from ._lib import check, lib, ptr, stream
from .resample import resample, resample_adjoint, resampled_length

MAX_ORDER = 16


def prepare_iir(b, a):
    """(b, a) of any array-like -> (bn, an) float32 CPU tensors, normalised by a[0] in float32 as lfilter does.
    Raises ValueError for an order above MAX_ORDER, len(b) != len(a), or a denominator with a root of modulus >= 1 (found in
    float64 on the float32-normalised coefficients: there the reference's own float32 filter diverges)."""
    bt = torch.as_tensor(np.asarray(b, dtype=np.float64).reshape(-1)).float()
    at = torch.as_tensor(np.asarray(a, dtype=np.float64).reshape(-1)).float()
    if bt.numel() != at.numel():
        raise ValueError(f"IIR filter: len(b) = {bt.numel()} != len(a) = {at.numel()} (lfilter requires equal lengths)")
    order = at.numel() - 1
    if order < 1:
        raise ValueError("IIR filter: order 0 (a must have at least two coefficients)")
    if order > MAX_ORDER:
        raise ValueError(f"IIR filter: order {order} above the supported limit of {MAX_ORDER}")
    if float(at[0]) == 0.0:
        raise ValueError("IIR filter: a[0] == 0")
    bn = bt / at[0:1]
    an = at / at[0:1]
    radius = float(np.abs(np.roots(an.double().numpy())).max())
    if not radius < 1.0:
        raise ValueError(f"IIR filter is unstable at float32 coefficients: largest pole radius {radius:.6f} >= 1")
    return bn.contiguous(), an.contiguous()


def iir_filter(x, b, a, clamp=False, adjoint=False, mask=None, prepared=False):
    """torchaudio.functional.lfilter(x, a, b, clamp) on x [B, L] (device, float32), or with adjoint=True its transpose
    reverse(lfilter(reverse(x))).  b, a: coefficients (normalised here unless prepared=True, then float32 tensors as
    prepare_iir returns them, on any device).  clamp: forward output clipped to [-1, 1]; a uint8 `mask` [B, L] then receives
    (|y| <= 1) in the forward and is REQUIRED by the adjoint, which zeroes its seed where the mask is 0."""
    if not x.is_cuda:
        raise RuntimeError("babe_amd.iir_filter runs on the GPU only (no CPU fallback)")
    if not prepared:
        b, a = prepare_iir(b, a)
    dev = x.device
    b = b.to(dev, torch.float32).contiguous()
    a = a.to(dev, torch.float32).contiguous()
    order = a.numel() - 1
    shape = x.shape
    xx = x.reshape(-1, shape[-1]).contiguous().float()
    B, L = xx.shape
    if clamp and adjoint and mask is None:
        raise ValueError("iir_filter: the clamped adjoint needs the forward's mask")
    if mask is not None and (mask.dtype != torch.uint8 or tuple(mask.shape) != (B, L) or not mask.is_contiguous()):
        raise ValueError(f"iir_filter: mask must be a contiguous uint8 tensor of shape {(B, L)}")
    out = torch.empty_like(xx)
    nbytes = int(lib().babe_iir_workspace(B, L, order))
    ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    with torch.cuda.device(dev):
        check(lib().babe_iir_filter(ptr(xx), xx.stride(0), ptr(out), out.stride(0), B, L, ptr(b), ptr(a), order, int(bool(clamp)),
                                    int(bool(adjoint)), ptr(mask) if (clamp and mask is not None) else None,
                                    mask.stride(0) if mask is not None else 0, ptr(ws), nbytes, stream(xx)), "iir_filter")
    return out.reshape(shape)


def decimated_length(L, factor):
    """len(range(0, L - 1, factor)): x[..., 0:-1:factor] drops the last sample."""
    return len(range(0, int(L) - 1, int(factor)))


def decimate(x, factor, adjoint=False, length=None):
    """x[..., 0:-1:factor] on x [B, L] (device); adjoint=True: the zero-stuffing transpose of g [B, decimated_length(length)]
    back to [B, length]."""
    if not x.is_cuda:
        raise RuntimeError("babe_amd.decimate runs on the GPU only (no CPU fallback)")
    factor = int(factor)
    if factor < 1:
        raise ValueError(f"decimate: factor {factor} < 1")
    shape = x.shape
    xx = x.reshape(-1, shape[-1]).contiguous().float()
    B = xx.shape[0]
    if adjoint:
        if length is None:
            raise ValueError("decimate(adjoint=True) needs the length of the undecimated signal")
        L_full, L_dec = int(length), xx.shape[1]
        if decimated_length(L_full, factor) != L_dec:
            raise ValueError(f"decimate adjoint: {L_dec} samples do not come from {L_full} at factor {factor}")
        n_out = L_full
    else:
        L_full = xx.shape[1]
        L_dec = decimated_length(L_full, factor)
        n_out = L_dec
    out = torch.empty(B, n_out, device=xx.device, dtype=torch.float32)
    if L_dec > 0:
        with torch.cuda.device(xx.device):
            check(lib().babe_decimate(ptr(xx), xx.stride(0), ptr(out), out.stride(0), B, L_full, L_dec, factor, int(bool(adjoint)),
                                      stream(xx)), "decimate")
    else:
        out.zero_()
    return out.reshape(*shape[:-1], n_out)


# ---- the degradation objects BlindSampler runs: fwd = A, adj = A^T ---------------------------------------------------------
class IIRDegradation:
    """'cheby1' (clamp=False) or 'biquad' (clamp=True).  The clamp mask of the LAST forward is what adj() differentiates
    through - the sampler always runs A^T right after the A it belongs to."""

    def __init__(self, b, a, clamp, device):
        bn, an = prepare_iir(b, a)
        self.b, self.a = bn.to(device), an.to(device)
        self.clamp = bool(clamp)
        self.mask = None

    def fwd(self, x, keep_mask=True):
        mask = None
        if self.clamp and keep_mask:
            mask = torch.empty(x.shape, device=x.device, dtype=torch.uint8)
            self.mask = mask
        return iir_filter(x, self.b, self.a, clamp=self.clamp, mask=mask, prepared=True)

    def adj(self, g):
        return iir_filter(g, self.b, self.a, clamp=self.clamp, adjoint=True, mask=self.mask, prepared=True)


class ResampleDegradation:
    """'resample': torchaudio.functional.resample(x, orig_freq=int(100 factor), new_freq=100); y is shorter than x."""

    def __init__(self, factor, length):
        self.orig, self.new, self.length = int(100 * factor), 100, int(length)

    def out_length(self):
        return resampled_length(self.length, self.orig, self.new)

    def fwd(self, x, keep_mask=True):
        return resample(x, self.orig, self.new)

    def adj(self, g):
        return resample_adjoint(g, self.orig, self.new, self.length)


class DecimateDegradation:
    """'decimate': x[..., 0:-1:factor]; y is shorter than x."""

    def __init__(self, factor, length):
        self.factor, self.length = int(factor), int(length)

    def out_length(self):
        return decimated_length(self.length, self.factor)

    def fwd(self, x, keep_mask=True):
        return decimate(x, self.factor)

    def adj(self, g):
        return decimate(g, self.factor, adjoint=True, length=self.length)
