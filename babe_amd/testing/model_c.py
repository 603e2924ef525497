"""ctypes view of a library-built network (csrc/model.hip: babe_model_load and friends) - what a host without Python holds instead
of a UnetEngine, a CQT_nsgt, an STFTOps and a CEval -, and of the descriptor's observation model (observe: a degrade.py object
onto babe_eval_desc.obs_kind and its parameters) and the host helpers babe_firwin_kaiser / babe_iir_check.  Used by the tests
(tests/test_gpu_model_c.py, tests/test_gpu_obs_library.py) and tools/model_load_bench.py only: the samplers keep building their
descriptors from the Python engine."""
import ctypes as C

from .._cabi import EvalDesc, ModelSummary
from .._lib import BabeHipError, check, lib, stream


class LibraryModel:
    """babe_model_load_ex(path, precision) on the current device and stream; `close()` (or garbage collection) destroys it.
    precision: 'f32' | 'bf16' | 'bf16x3' (ops.PRECISIONS) - the host's choice, the file holds the fp32 masters.
    attention_precision: None - a file with time-attention layers is refused -, or the attention core such a file runs on, 'f32' |
    'bf16' (babe_model_load_opt), as the Python network's option of that name.  Plans and descriptors taken from it point into
    its arena: keep the object alive while they are in use."""

    def __init__(self, path, precision="f32", attention_precision=None):
        from .._cabi import ATTN_CORES, ModelOptions
        from ..ops import PRECISIONS
        if attention_precision is None:
            self.handle, who = lib().babe_model_load_ex(str(path).encode(), PRECISIONS[precision], stream()), "babe_model_load_ex"
        else:
            opt = ModelOptions(precision=PRECISIONS[precision], attention=ATTN_CORES[attention_precision])
            self.handle, who = lib().babe_model_load_opt(str(path).encode(), C.byref(opt), stream()), "babe_model_load_opt"
        if not self.handle:
            raise BabeHipError(who + ": " + lib().babe_last_error().decode())

    def close(self):
        if getattr(self, "handle", None):
            lib().babe_model_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def info(self):
        s = ModelSummary()
        check(lib().babe_model_info(self.handle, C.byref(s)), "model_info")
        return s

    @property
    def precision(self):
        """babe_model_precision: 0 f32, 1 bf16, 2 bf16x3."""
        return lib().babe_model_precision(self.handle)

    @property
    def attention(self):
        """babe_model_attention: 0 refused, 1 the fp32 core, 2 the bf16 core."""
        return lib().babe_model_attention(self.handle)

    def setting(self, key):
        v = C.c_double()
        check(lib().babe_model_setting(self.handle, key.encode(), C.byref(v)), "model_setting")
        return v.value

    @property
    def plan(self):
        """The library-side UNet plan (for babe_unet_workspace_bytes / babe_unet_fwd / babe_unet_vjp)."""
        p = lib().babe_model_unet_plan(self.handle)
        if not p:
            raise BabeHipError("babe_model_unet_plan: " + lib().babe_last_error().decode())
        return p

    @property
    def cqt_plan(self):
        p = lib().babe_model_cqt_plan(self.handle)
        if not p:
            raise BabeHipError("babe_model_cqt_plan: " + lib().babe_last_error().decode())
        return p

    def eval_desc(self, state):
        """A babe_eval_desc over this model and the caller's UNet state (babe_unet_state_create), every field filled."""
        d = EvalDesc()
        check(lib().babe_model_eval_desc(self.handle, state, C.byref(d)), "model_eval_desc")
        return d


class _PlanOwner:
    """What networks.unet_c.CUnet reads of an engine, over a library-built model."""

    def __init__(self, model):
        self._plan, self.nocts, self._handle = model, model.info.nocts, model.plan

    def c_plan(self):
        return self._handle


def unet(model):
    """A library-side UNet state and workspace (networks.unet_c.CUnet: fwd / vjp) over the model's own plan."""
    from ..networks.unet_c import CUnet
    return CUnet(_PlanOwner(model))


def edm_steps(model, T, snoise=1.0):
    """(rows, t0, warm_start) of a run of T steps from the file's tester.diff_params, by the library's double-precision schedule
    (babe_edm_steps) - what a host without the Python EDM class uses."""
    from .._cabi import SampleStep
    rows, t0 = (SampleStep * T)(), C.c_float()
    g = lambda k: model.setting("tester.diff_params." + k)
    try:
        start = model.setting("tester.posterior_sampling.start_sigma")
    except BabeHipError:                                 # "None" in the file: a cold start from sigma_max
        start = -1.0
    check(lib().babe_edm_steps(rows, C.byref(t0), T, int(model.setting("tester.order")), g("sigma_min"), g("sigma_max"), g("ro"),
                               g("sigma_data"), g("Schurn"), g("Stmin"), g("Stmax"), float(snoise), start), "edm_steps")
    return rows, t0.value, start > 0


def observe(desc, degradation, dc_classic=False):
    """The known observation model `degradation` (babe_amd/degrade.py: FIRDegradation, IIRDegradation, MaskDegradation,
    ClipDegradation, or MaskMixDegradation over a FIR or over None = the STFT filter; None = the STFT filter alone) into the
    babe_eval_desc `desc`, with blind = 0 for every known one; dc_classic: the replacement step x0 <- y + x0 - A(x0).  The tensors
    whose addresses the descriptor now holds stay alive with it (desc._keep; a copy by value, as into a babe_sample_desc, does not
    carry them: keep `desc` itself while the copy is in use).  Returns desc."""
    from .._cabi import OBS_CLIP, OBS_FIR, OBS_IIR, OBS_MASK, OBS_STFT
    from .._lib import ptr
    from ..degrade import ClipDegradation, FIRDegradation, IIRDegradation, MaskDegradation, MaskMixDegradation
    d, keep = desc, []
    d.obs_kind, d.taps, d.ntaps, d.b, d.a, d.order, d.clamp = OBS_STFT, None, 0, None, None, 0, 0
    d.obs_mask, d.obs_mask_bs, d.clip_value, d.dc_classic = None, 0, 0.0, int(bool(dc_classic))
    d.mask, d.mask_bs = None, 0

    def rows(m):              # ([L] or [B,L] float32 rows, their stride: 0 = one row for every clip)
        m = m.float().contiguous()
        keep.append(m)
        return ptr(m), (0 if m.dim() == 1 or m.shape[0] == 1 else m.stride(0))

    deg = degradation
    if isinstance(deg, MaskMixDegradation):
        d.mask, d.mask_bs = rows(deg.mask)
        deg = deg.inner
        if deg is not None and not isinstance(deg, FIRDegradation):
            raise NotImplementedError("the AR mix runs over the STFT filter or a FIR")
    if deg is None:
        pass
    elif isinstance(deg, FIRDegradation):
        keep.append(deg.taps)
        d.obs_kind, d.taps, d.ntaps = OBS_FIR, ptr(deg.taps), deg.taps.numel()
    elif isinstance(deg, IIRDegradation):
        keep.extend([deg.b, deg.a])
        d.obs_kind, d.b, d.a, d.order, d.clamp = OBS_IIR, ptr(deg.b), ptr(deg.a), deg.a.numel() - 1, int(deg.clamp)
    elif isinstance(deg, MaskDegradation):
        d.obs_kind = OBS_MASK
        d.obs_mask, d.obs_mask_bs = rows(deg.mask)
    elif isinstance(deg, ClipDegradation):
        d.obs_kind, d.clip_value = OBS_CLIP, deg.c
    else:
        raise NotImplementedError(f"{type(deg).__name__}: the observation is not of the state's shape, or has no library-side "
                                  f"sequencing")
    if degradation is not None:
        d.blind = 0
    desc._keep = keep
    return desc


def firwin_kaiser(numtaps, cutoff, width, fs, highpass=False):
    """babe_firwin_kaiser -> the taps as a float64 numpy array (scipy.signal.firwin(..., width=width, window='kaiser', fs=fs))."""
    import numpy as np
    taps = np.empty(int(numtaps), dtype=np.float64)
    check(lib().babe_firwin_kaiser(int(numtaps), float(cutoff), float(width), float(fs), int(bool(highpass)), taps.ctypes.data),
          "firwin_kaiser")
    return taps


def iir_check(b, a):
    """babe_iir_check on float32 coefficients already divided by a[0] -> (ok, message).  One `order` describes both arrays in the
    C call, so arrays of different lengths - which degrade.prepare_iir refuses - have no call to make: refused here."""
    import numpy as np
    b, a = np.ascontiguousarray(b, dtype=np.float32).reshape(-1), np.ascontiguousarray(a, dtype=np.float32).reshape(-1)
    if b.size != a.size:
        return False, f"len(b) = {b.size} != len(a) = {a.size}"
    rc = lib().babe_iir_check(b.ctypes.data, a.ctypes.data, a.size - 1)
    return rc == 0, ("" if rc == 0 else lib().babe_last_error().decode())


def sample(model, state, y, params, rows, t0, warm_start, seed, clip0=0, blind=True, desc=None, noise=None, skip_zero_inject=False,
           shape=None):
    """babe_sample_bwe on the model's descriptor: y [B,L] (None: unconditional sampling of `shape` = (B, L)), params [P,2,K] (left
    alone; None where the descriptor's observation model is not the STFT filter), the noise from the library's generator under
    (seed, clip0) or, with noise [T+1,B,L], from that buffer; skip_zero_inject: a step with inject == 0 evaluates the state as it
    is -> (x, params, the babe_sample_desc used)."""
    import torch
    from .._cabi import SampleDesc
    from .._lib import ptr
    T = len(rows)
    B, L = y.shape if y is not None else shape
    d = SampleDesc()
    d.eval = desc if desc is not None else model.eval_desc(state)
    if params is not None:
        d.eval.K = int(params.shape[-1])
    d.eval.blind = int(bool(blind))
    d.T, d.steps, d.t0, d.warm_start, d.skip_zero_inject = T, rows, t0, int(bool(warm_start)), int(bool(skip_zero_inject))
    n = lib().babe_sample_workspace_bytes(C.byref(d), B)
    if n < 0:
        raise BabeHipError("sample_workspace_bytes: " + lib().babe_last_error().decode())
    dev = y.device if y is not None else torch.device("cuda", torch.cuda.current_device())
    ws = torch.empty(n, device=dev, dtype=torch.uint8)
    p = params.clone().contiguous() if params is not None else None
    x = torch.empty((B, L), device=dev, dtype=torch.float32)
    if noise is not None:
        assert noise.shape == (T + 1, B, L) and noise.is_contiguous() and noise.dtype == torch.float32 and noise.device == dev
    check(lib().babe_sample_bwe(C.byref(d), ptr(y), ptr(p), ptr(x), ptr(noise), int(seed), int(clip0), None, None, ptr(ws), n, B,
                                stream()), "sample_bwe")
    torch.cuda.synchronize(dev)                          # ws is released on return
    return x, p, d
