"""Known low-pass degradations of the tester.  Mirrors the reference's utils/bandwidth_extension.py under its own names and
return structures: prepare_filter :7-39 (filter design from tester.bandwidth_extension, host side exactly like the reference),
get_FIR_lowpass / get_FIR_high_pass (scipy.signal.firwin), get_cheby1_ba (scipy.signal.cheby1), design_biquad_lpf (float32
torch math) and apply_low_pass with its per-type helpers - there on ATen / torchaudio, here on the HIP kernels
(babe_fir_same, csrc/degrade.hip, csrc/resample_sinc.hip)."""
import math

import scipy.signal
import torch

from ..degrade import decimate, iir_filter
from ..resample import resample
from ..stft import fir_same


def prepare_filter(args, sample_rate):
    """The filter the tester feeds predict_bwe for tester.bandwidth_extension.filter.type (:7-39).  Like the reference,
    'decimate' writes filter.resample.fs = int(sample_rate / factor) back into args."""
    bwe = args.tester.bandwidth_extension
    order, fc, ftype = bwe.filter.order, bwe.filter.fc, bwe.filter.type
    if ftype == "firwin":
        return get_FIR_lowpass(order, fc, bwe.filter.beta, sample_rate)
    if ftype == "firwin_hpf":
        return get_FIR_high_pass(order, fc, bwe.filter.beta, sample_rate)
    if ftype == "cheby1":
        return get_cheby1_ba(order, bwe.filter.ripple, 2 * fc / sample_rate)
    if ftype == "biquad":
        return design_biquad_lpf(fc, sample_rate, bwe.filter.biquad.Q)
    if ftype == "resample":
        return sample_rate / bwe.filter.resample.fs
    if ftype == "decimate":
        factor = int(bwe.decimate.factor)
        bwe.filter.resample.fs = int(sample_rate / factor)
        return factor
    raise NotImplementedError(ftype)        # cheby1filtfilt, butter_fir, cheby1_fir and unknown types raise there too


def get_FIR_lowpass(order, fc, beta, sr):
    B = scipy.signal.firwin(numtaps=order, cutoff=fc, width=beta, window="kaiser", fs=sr)
    return torch.FloatTensor(B).unsqueeze(0).unsqueeze(0)


def get_FIR_high_pass(order, fc, beta, sr):
    B = scipy.signal.firwin(numtaps=order - 1, cutoff=fc, width=beta, window="kaiser", fs=sr, pass_zero="highpass")
    return torch.FloatTensor(B).unsqueeze(0).unsqueeze(0)


def get_cheby1_ba(order, ripple, hi):
    """(b, a) float64 numpy arrays of scipy.signal.cheby1(order, ripple, hi, btype='lowpass', output='ba')."""
    b, a = scipy.signal.cheby1(order, ripple, hi, btype="lowpass", output="ba")
    return b, a


def design_biquad_lpf(fc, fs, Q):
    """(b0, b1, b2, a0, a1, a2) as 0-d float32 tensors, the reference's float32 torch arithmetic."""
    w0 = torch.as_tensor(2 * math.pi * fc / fs, dtype=torch.float32)
    alpha = torch.sin(w0) / 2 / Q
    b0 = (1 - torch.cos(w0)) / 2
    b1 = 1 - torch.cos(w0)
    b2 = b0
    a0 = 1 + alpha
    a1 = -2 * torch.cos(w0)
    a2 = 1 - alpha
    return b0, b1, b2, a0, a1, a2


def apply_low_pass_firwin(y, filter):
    return fir_same(y.contiguous().float(), filter.to(y.device))


def apply_low_pass_IIR(y, filter):
    b, a = filter
    return iir_filter(y.contiguous().float(), b, a, clamp=False)


def apply_low_pass_biquad(y, filter):
    c = [float(torch.as_tensor(v).reshape(-1)[0]) for v in filter]
    return iir_filter(y.contiguous().float(), torch.tensor(c[:3]), torch.tensor(c[3:]), clamp=True)


def apply_decimate(y, factor):
    return decimate(y, factor)


def apply_resample(y, factor):
    N = 100
    return resample(y, orig_freq=int(factor * N), new_freq=N)


def apply_low_pass(y, filter, type):
    """Dispatch on the filter type (:141-163); an unknown type returns None, as there."""
    if type in ("firwin", "firwin_hpf"):
        return apply_low_pass_firwin(y, filter)
    if type == "cheby1":
        return apply_low_pass_IIR(y, filter)
    if type == "biquad":
        return apply_low_pass_biquad(y, filter)
    if type == "resample":
        return apply_resample(y, filter)
    if type == "decimate":
        return apply_decimate(y, filter)
    return None
