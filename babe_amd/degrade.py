"""The observation models y = A(x) the samplers guide against, each an object of one protocol (class Degradation below), and
the kernels of the reference's 'cheby1' (torchaudio.functional.lfilter, clamp=False), 'biquad' (torchaudio.functional.biquad:
lfilter with its default clamp=True), 'resample' (torchaudio.functional.resample(x, int(100 factor), 100)) and 'decimate'
(x[..., 0:-1:factor]), testing/blind_bwe_sampler.py:219-230 - forward A and adjoint A^T on the HIP kernels of csrc/degrade.hip.

Coefficients are prepared on the host the way lfilter sees them: rounded to float32 (`torch.Tensor(b)`), divided by a[0] in
float32.  The recursion itself runs in float64 on the GPU.  Device tensors only, no CPU fallback."""
import numpy as np
import torch

from ._lib import check, lib, ptr, stream
from .resample import resample, resample_adjoint, resampled_length
from .stft import STFTOps, fir_same, lincomb, mask_blend

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


def sumsq_partial(g, nblk=STFTOps.NBLK):
    """Per-block partial sums of squares of g [B, n] -> [B, nblk] float64 (fixed-order: what the norm kernels reduce)."""
    B, n = g.shape
    part = torch.empty(B, nblk, device=g.device, dtype=torch.float64)
    check(lib().babe_sumsq_partial(ptr(g), g.stride(0), ptr(part), nblk, B, n, stream()), "sumsq_partial")
    return part


# ---- the degradation objects the samplers run ----------------------------------------------------------------------------
class Degradation:
    """One observation model: fwd = A, adj = A^T, and the two compositions a score evaluation makes of them."""

    post = False        # True: the guidance seed carries the overlap-add envelope (the STFT filter alone)

    def residual(self, x, y):
        """(r = y - A(x), the per-block sums of r^2 the guidance seed normalises with)."""
        r = lincomb(torch.empty_like(y), 1.0, y, -1.0, self.fwd(x))
        return r, sumsq_partial(r)

    def guidance(self, x, y, seed):
        """A^T applied to d(distance)/d(rec) at rec = A(x); seed(r, y, part, post) is the sampler's distance gradient.  y (and r,
        the seed) may be shorter than x ('resample' / 'decimate'): A^T maps back to x's length."""
        r, part = self.residual(x, y)
        return self.adj(seed(r, y, part, self.post))

    def fwd_dc(self, x):
        """A(x) of the replacement data-consistency step x0 <- y + x0 - A(x0)."""
        return self.fwd(x)

    def bind(self, st, filter_params, B):
        """This degradation for one evaluation (only a mix over the STFT filter depends on the evaluation's filter_params)."""
        return self


class FIRDegradation(Degradation):
    """'firwin' / 'firwin_hpf': F.conv1d(padding="same") with the taps (:211-218; edm_sampler.py:245-252)."""

    def __init__(self, taps, device):
        self.taps = torch.as_tensor(taps, dtype=torch.float32).reshape(-1).contiguous().to(device)

    def fwd(self, x):
        return fir_same(x, self.taps)

    def adj(self, g):
        return fir_same(g, self.taps, adjoint=True)


class MaskDegradation(Degradation):
    """A(x) = mask * x of edm_sampler.Sampler.predict_inpainting (edm_sampler.py:231-243); mask [L] or [B,L], self-adjoint."""

    def __init__(self, mask, device):
        self.mask = torch.as_tensor(mask, dtype=torch.float32).contiguous().to(device)

    def fwd(self, x):
        return mask_blend(self.mask, x, None)

    adj = fwd


class STFTFilterDegradation(Degradation):
    """The piecewise STFT-domain filter of filter_params [2,K] or [P,2,K] (blind and 'fc_A'; one filter per clip of the batch of B,
    or one shared), built per evaluation.  spec: the STFT of the signal residual() will see, where the caller has taken it
    already (the blind fit needs it first).  adj is the transpose up to the overlap-add envelope, which the seed carries."""

    post = True

    def __init__(self, st, filter_params, B, spec=None):
        H = st.design_filter(torch.as_tensor(filter_params, dtype=torch.float32, device=st.dev))
        self.st, self.spec, self.H = st, spec, H if (H.dim() == 1 or H.shape[0] == B) else H[0]

    def _apply(self, spec, normalise, y=None):
        return self.st.ola(self.st.filter_frames(spec, self.H), normalise=normalise, y=y)

    def fwd(self, x):
        return self._apply(self.st.stft(x), True)

    def adj(self, g):
        return self._apply(self.st.stft(g), False)

    def residual(self, x, y):
        return self._apply(self.spec if self.spec is not None else self.st.stft(x), True, y)      # (fused into the overlap-add)


class MaskMixDegradation(Degradation):
    """predict_bwe_AR (:280-288): mask*x + (1-mask)*A(x) with A = `inner` - a FIRDegradation, or None for the STFT filter of
    the evaluation's filter_params ('fc_A'), which bind() builds."""

    def __init__(self, mask, inner):
        self.mask, self.inner = mask, inner

    def bind(self, st, filter_params, B):
        return self if self.inner is not None else MaskMixDegradation(self.mask, STFTFilterDegradation(st, filter_params, B))

    def fwd(self, x):
        return mask_blend(self.mask, x, self.inner.fwd(x))

    def guidance(self, x, y, seed):
        r, part = self.residual(x, y)
        s = seed(r, y, part, False)                                      # -r/||r||: the observed part takes it as it is
        gA = self.inner.adj(mask_blend(self.mask, None, seed(r, y, part, True) if self.inner.post else s))
        return lincomb(torch.empty_like(gA), 1.0, mask_blend(self.mask, s, None), 1.0, gA)

    def fwd_dc(self, x):
        # The classic replacement step of an AR run (posterior_sampling.data_consistency on, inpaint_DC off) applies the inner
        # filter WITHOUT the mask mix the guidance uses (the reference has no working step in that configuration).  Kept as is.
        return self.inner.fwd(x)


class IIRDegradation(Degradation):
    """'cheby1' (clamp=False) or 'biquad' (clamp=True).  The clamp mask of the LAST forward is what adj() differentiates
    through - the sampler always runs A^T right after the A it belongs to."""

    def __init__(self, b, a, clamp, device):
        bn, an = prepare_iir(b, a)
        self.b, self.a = bn.to(device), an.to(device)
        self.clamp = bool(clamp)
        self.mask = None

    def fwd(self, x):
        mask = None
        if self.clamp:
            mask = torch.empty(x.shape, device=x.device, dtype=torch.uint8)
            self.mask = mask
        return iir_filter(x, self.b, self.a, clamp=self.clamp, mask=mask, prepared=True)

    def adj(self, g):
        return iir_filter(g, self.b, self.a, clamp=self.clamp, adjoint=True, mask=self.mask, prepared=True)


class ResampleDegradation(Degradation):
    """'resample': torchaudio.functional.resample(x, orig_freq=int(100 factor), new_freq=100); y is shorter than x."""

    def __init__(self, factor, length):
        self.orig, self.new, self.length = int(100 * factor), 100, int(length)

    def out_length(self):
        return resampled_length(self.length, self.orig, self.new)

    def fwd(self, x):
        return resample(x, self.orig, self.new)

    def adj(self, g):
        return resample_adjoint(g, self.orig, self.new, self.length)


class DecimateDegradation(Degradation):
    """'decimate': x[..., 0:-1:factor]; y is shorter than x."""

    def __init__(self, factor, length):
        self.factor, self.length = int(factor), int(length)

    def out_length(self):
        return decimated_length(self.length, self.factor)

    def fwd(self, x):
        return decimate(x, self.factor)

    def adj(self, g):
        return decimate(g, self.factor, adjoint=True, length=self.length)


def clip_residual(x, y, clip_value, nblk=STFTOps.NBLK):
    """One pass over x, y [B, L] (device): (r = y - clip(x, -c, c), mask uint8 = |x| <= c, the block sums sumsq_partial(r) gives)."""
    if not (x.is_cuda and y.is_cuda):
        raise RuntimeError("babe_amd.clip_residual runs on the GPU only (no CPU fallback)")
    B, L = x.shape
    assert y.shape == x.shape and x.stride(1) == 1 and y.stride(1) == 1
    r = torch.empty(B, L, device=x.device, dtype=torch.float32)
    mask = torch.empty(B, L, device=x.device, dtype=torch.uint8)
    part = torch.empty(B, nblk, device=x.device, dtype=torch.float64)
    with torch.cuda.device(x.device):
        check(lib().babe_clip_residual(ptr(x), x.stride(0), ptr(y), y.stride(0), float(clip_value), ptr(r), r.stride(0), ptr(mask),
                                       mask.stride(0), ptr(part), nblk, B, L, stream(x)), "clip_residual")
    return r, mask, part


SPECNORM_ITERS = 32


def specnorm_seed(r, rows, cols, iters=SPECNORM_ITERS):
    """d s1(R) / d(rec) = -u1 v1^T for the residual r [B, rows * cols] = y - rec (device), s1 the largest singular value of
    R = r[b] as [rows, cols]: the gradient of torch.linalg.norm(y - rec, dim=(1, 2), ord=2).  `iters` power iterations on R^T R
    from u = ones; the error shrinks by (s2 / s1)^2 per iteration (32 reach float32 for s2 / s1 <= 0.75; where the two
    largest singular values coincide the gradient does not exist, in torch either)."""
    if not r.is_cuda:
        raise RuntimeError("babe_amd.specnorm_seed runs on the GPU only (no CPU fallback)")
    B = r.shape[0]
    r = r.reshape(B, -1).contiguous()
    if r.shape[1] != rows * cols:
        raise ValueError(f"specnorm_seed: r has {r.shape[1]} entries per row, expected {rows} x {cols}")
    out = torch.empty_like(r)
    nbytes = int(lib().babe_specnorm_workspace(B, rows, cols))
    ws = torch.empty(nbytes, device=r.device, dtype=torch.uint8)
    with torch.cuda.device(r.device):
        check(lib().babe_specnorm_seed(ptr(r), r.stride(0), rows, cols, int(iters), ptr(out), out.stride(0), B, ptr(ws), nbytes,
                                       stream(r)), "specnorm_seed")
    return out


def stft_mag_frames(length, hop):
    """Frames of torch.stft(cat(x, zeros(win)), win, hop, center=False) on `length` samples: 1 + length // hop."""
    return 1 + int(length) // int(hop)


class ClipDegradation(Degradation):
    """Declipping: A(x) = clip(x, -c, c).  adj multiplies by the mask |x| <= c of the LAST forward or residual (torch.clip's
    gradient: 1 on the closed interval, 0 outside) - the sampler always runs A^T right after the A it belongs to."""

    def __init__(self, clip_value):
        self.c = float(clip_value)
        if not self.c >= 0.0:
            raise ValueError(f"ClipDegradation: clip_value {clip_value!r} must be >= 0")
        self.mask = None

    def fwd(self, x):
        if not x.is_cuda:
            raise RuntimeError("babe_amd.ClipDegradation runs on the GPU only (no CPU fallback)")
        x = x.contiguous()
        out = torch.empty_like(x)
        self.mask = None                      # (the plain forward leaves no mask: residual() is what precedes adj)
        with torch.cuda.device(x.device):
            check(lib().babe_clip_fwd(ptr(x), x.stride(0), self.c, ptr(out), out.stride(0), x.shape[0], x.shape[1], stream(x)),
                  "clip_fwd")
        return out

    def residual(self, x, y):
        r, self.mask, part = clip_residual(x.contiguous(), y.contiguous(), self.c)       # (fused: one pass)
        return r, part

    def adj(self, g):
        if self.mask is None or tuple(self.mask.shape) != tuple(g.shape):
            raise ValueError("ClipDegradation.adj: needs the mask of a residual() on a signal of this shape")
        g = g.contiguous()
        out = torch.empty_like(g)
        with torch.cuda.device(g.device):
            check(lib().babe_clip_adj(ptr(g), g.stride(0), ptr(self.mask), self.mask.stride(0), ptr(out), out.stride(0), g.shape[0],
                                      g.shape[1], stream(g)), "clip_adj")
        return out


class STFTMagnitudeDegradation(Degradation):
    """Phase retrieval: A(x) = |torch.stft(cat(x, zeros(win)), win, hop, hamming_window(win), center=False)| on x [B, length],
    flattened to [B, bins * frames] (bins = win/2 + 1 major, frames = 1 + length // hop: torch.stft's layout) so that the norm and
    seed kernels take it as a signal.  adj(g) is the vector-Jacobian product at the x of the LAST fwd, whose spectrum it keeps.
    Where a bin is exactly zero the VJP is DEFINED as 0: torch's sqrt(re^2 + im^2) has a NaN gradient there, which the reference
    returns whenever a frame lies wholly in the zero padding (length % hop == 0)."""

    def __init__(self, win, hop, length, device, matrix_norm=False):
        """matrix_norm: guidance() differentiates the MATRIX 2-norm of the bins x frames residual (its largest singular value),
        which is what the reference's torch.linalg.norm(y - A(x), dim=(1, 2), ord=2) computes for its 3-D observation, and
        ignores the sampler's seed; False: the sampler's distance on the flattened residual, like every other degradation."""
        self.matrix_norm = bool(matrix_norm)
        win, hop, length = int(win), int(hop), int(length)
        if win < 256 or win > 4096 or win & (win - 1):
            raise ValueError(f"STFTMagnitudeDegradation: win = {win} is not a power of two in 256...4096")
        if not 1 <= hop <= win:
            raise ValueError(f"STFTMagnitudeDegradation: hop = {hop} outside 1...win = {win}")
        if length < 1:
            raise ValueError(f"STFTMagnitudeDegradation: length = {length} < 1")
        self.win, self.hop, self.length, self.dev = win, hop, length, torch.device(device)
        self.bins, self.frames = win // 2 + 1, stft_mag_frames(length, hop)
        self.spec = None
        self._tables = None

    def out_shape(self):
        return (self.bins, self.frames)

    def _tab(self):
        if self.dev.type != "cuda":
            raise RuntimeError("babe_amd.STFTMagnitudeDegradation runs on the GPU only (no CPU fallback)")
        if self._tables is None:
            q = np.arange(2048, dtype=np.float64)
            tw = torch.tensor(np.stack([np.cos(2 * np.pi * q / 4096), -np.sin(2 * np.pi * q / 4096)], -1), dtype=torch.float32)
            window = torch.hamming_window(self.win, dtype=torch.float32)           # periodic, float32, like the reference
            self._tables = (window.to(self.dev), tw.contiguous().to(self.dev))
        return self._tables

    def fwd(self, x):
        if not x.is_cuda:
            raise RuntimeError("babe_amd.STFTMagnitudeDegradation runs on the GPU only (no CPU fallback)")
        if x.dim() != 2 or x.shape[1] != self.length:
            raise ValueError(f"STFTMagnitudeDegradation.fwd: x of shape {tuple(x.shape)}, expected [B, {self.length}]")
        window, tw = self._tab()
        x = x.contiguous()
        B = x.shape[0]
        self.spec = torch.empty(B, self.frames, self.bins, 2, device=x.device, dtype=torch.float32)
        mag = torch.empty(B, self.bins * self.frames, device=x.device, dtype=torch.float32)
        with torch.cuda.device(x.device):
            check(lib().babe_stft_mag_fwd(ptr(x), x.stride(0), self.length, ptr(window), self.win, self.hop, ptr(self.spec), ptr(mag),
                                          B, self.frames, ptr(tw), stream(x)), "stft_mag_fwd")
        return mag

    def adj(self, g):
        if not g.is_cuda:
            raise RuntimeError("babe_amd.STFTMagnitudeDegradation runs on the GPU only (no CPU fallback)")
        B = g.shape[0]
        if self.spec is None or self.spec.shape[0] != B or g.numel() != B * self.bins * self.frames:
            raise ValueError("STFTMagnitudeDegradation.adj: needs the spectrum of a fwd() on a batch of this size")
        window, tw = self._tab()
        g = g.reshape(B, -1).contiguous()
        gx = torch.empty(B, self.length, device=g.device, dtype=torch.float32)
        nbytes = int(lib().babe_stft_mag_workspace(B, self.frames, self.win))
        ws = torch.empty(nbytes, device=g.device, dtype=torch.uint8)
        with torch.cuda.device(g.device):
            check(lib().babe_stft_mag_vjp(ptr(g), ptr(self.spec), ptr(window), self.win, self.hop, ptr(gx), gx.stride(0), self.length,
                                          B, self.frames, ptr(tw), ptr(ws), nbytes, stream(g)), "stft_mag_vjp")
        return gx

    def guidance(self, x, y, seed):
        if not self.matrix_norm:
            return super().guidance(x, y, seed)
        r = lincomb(torch.empty_like(y), 1.0, y, -1.0, self.fwd(x))
        return self.adj(specnorm_seed(r, self.bins, self.frames))

    def fwd_dc(self, x):
        raise NotImplementedError("STFTMagnitudeDegradation: no data-consistency step (the reference calls "
                                  "data_consistency_step_phase_retrieval, which it never defines)")


def make_degradation(filt, filt_type, device, length=None):
    """(filt, filt_type) of predict_bwe / predict_bwe_AR -> (degradation, filter_params [1,2,K] on `device`); the degradation is
    None for 'fc_A', the STFT filter of the returned filter_params.  length: the state's, for 'resample' / 'decimate'."""
    if filt_type == "fc_A":
        p = torch.as_tensor(filt, dtype=torch.float32)
        return None, (p.unsqueeze(1) if p.dim() == 1 else p).unsqueeze(0).contiguous().to(device)
    if filt_type in ("firwin", "firwin_hpf"):
        deg = FIRDegradation(filt, device)
    elif filt_type == "cheby1":
        deg = IIRDegradation(*filt, clamp=False, device=device)
    elif filt_type == "biquad":
        c6 = [float(torch.as_tensor(v).reshape(-1)[0]) for v in filt]       # torch.Tensor(b0) ... as float32 (:228-236)
        deg = IIRDegradation(c6[:3], c6[3:], clamp=True, device=device)
    elif filt_type in ("resample", "decimate"):
        deg = (ResampleDegradation if filt_type == "resample" else DecimateDegradation)(filt, length)
    else:
        raise NotImplementedError(f"filt_type={filt_type!r}: 'fc_A', 'firwin', 'firwin_hpf', 'cheby1', 'biquad', 'resample' and "
                                  f"'decimate' run on the HIP path")
    return deg, torch.zeros(1, 2, 1, device=device)
