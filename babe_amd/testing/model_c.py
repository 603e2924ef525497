"""ctypes view of a library-built network (csrc/model.hip: babe_model_load and friends) - what a host without Python holds instead
of a UnetEngine, a CQT_nsgt, an STFTOps and a CEval.  Used by tests/test_gpu_model_c.py and tools/model_load_bench.py only: the
samplers keep building their descriptors from the Python engine."""
import ctypes as C

from .._cabi import EvalDesc, ModelSummary
from .._lib import BabeHipError, check, lib, stream


class LibraryModel:
    """babe_model_load_ex(path, precision) on the current device and stream; `close()` (or garbage collection) destroys it.
    precision: 'f32' | 'bf16' | 'bf16x3' (ops.PRECISIONS) - the host's choice, the file holds the fp32 masters.  Plans and
    descriptors taken from it point into its arena: keep the object alive while they are in use."""

    def __init__(self, path, precision="f32"):
        from ..ops import PRECISIONS
        self.handle = lib().babe_model_load_ex(str(path).encode(), PRECISIONS[precision], stream())
        if not self.handle:
            raise BabeHipError("babe_model_load_ex: " + lib().babe_last_error().decode())

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


def sample(model, state, y, params, rows, t0, warm_start, seed, clip0=0, blind=True, desc=None):
    """babe_sample_bwe on the model's descriptor: y [B,L], params [P,2,K] (left alone), the noise from the library's generator
    under (seed, clip0) -> (x, params, the babe_sample_desc used)."""
    import torch
    from .._cabi import SampleDesc
    from .._lib import ptr
    B, T = y.shape[0], len(rows)
    d = SampleDesc()
    d.eval = desc if desc is not None else model.eval_desc(state)
    d.eval.K, d.eval.blind = int(params.shape[-1]), int(bool(blind))
    d.T, d.steps, d.t0, d.warm_start = T, rows, t0, int(bool(warm_start))
    n = lib().babe_sample_workspace_bytes(C.byref(d), B)
    if n < 0:
        raise BabeHipError("sample_workspace_bytes: " + lib().babe_last_error().decode())
    ws = torch.empty(n, device=y.device, dtype=torch.uint8)
    p, x = params.clone().contiguous(), torch.empty_like(y)
    check(lib().babe_sample_bwe(C.byref(d), ptr(y), ptr(p), ptr(x), None, int(seed), int(clip0), None, None, ptr(ws), n, B, stream()),
          "sample_bwe")
    torch.cuda.synchronize(y.device)                     # ws is released on return
    return x, p, d
