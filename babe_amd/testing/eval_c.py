"""BABE_EVAL_C=1: BlindSampler.evaluate as ONE call into the library (csrc/score_eval.hip, babe_score_eval) - the path a
non-Python host takes: UNet plan + state (csrc/unet_engine.hip), CQT plan (csrc/cqt_plan.hip), the STFT tables and the sampler's
scalars in a babe_eval_desc.  The default configuration (what predict_blind_bwe / predict_bwe(..., 'fc_A') run with the formal
tester YAMLs) and the observation model of predict_bwe_AR(..., 'fc_A'); everything else stays with the Python sequencer.
Bit-identical to it: tests/test_gpu_eval_c.py, tests/test_gpu_sample_ar_c.py."""
import ctypes as C

import torch

from .._cabi import EvalDesc
from .._lib import check, lib, ptr, stream, workspace
from ..cqt import MAX_BAND
from ..degrade import MaskMixDegradation


def cqt_plan_of(cq):
    """The library-side plan of a CQT_nsgt object: its own (the default), or one made here for an object that sequences the kernels
    itself (BABE_CQT_C=0); None where the library cannot plan the length."""
    if getattr(cq, "_plan", None):
        return cq._plan
    if not cq.fft.mixed:                                   # BABE_FFT_MIXED=0 / an uncovered length: the plan has no dense form
        return None
    if getattr(cq, "_plan_eval", None) is None:
        cq._plan_eval = lib().babe_cqt_plan_create_ex(float(cq.fs), cq.Ls, cq.numocts, cq.binsoct, float(cq.design["beta"]), MAX_BAND) or 0
    return cq._plan_eval or None


def _rows_ok(m, y):
    """A mask-like tensor babe_score_eval reads: float32 on y's device, [L], [1,L] or [B,L] with unit element stride."""
    return (torch.is_tensor(m) and m.dtype == torch.float32 and m.device == y.device and m.dim() in (1, 2) and m.stride(-1) == 1
            and m.shape[-1] == y.shape[-1] and (m.dim() == 1 or m.shape[0] in (1, y.shape[0])))


def _observation_ok(smp, y, blind):
    """The observation models the call sequences: the STFT filter alone (no degradation object, no replacement step), or the
    mask mix of predict_bwe_AR over it with, optionally, the (smooth_mask, y_smooth_masked) pair of inpaint_DC.  smp.dc takes
    precedence over the data_consistency attribute, as in BlindSampler.evaluate."""
    deg, dc = smp.degradation, smp.dc
    if deg is None:
        return dc is None and not (smp._dc_cfg if blind else smp.data_consistency)
    if blind or not isinstance(deg, MaskMixDegradation) or deg.inner is not None or not _rows_ok(deg.mask, y):
        return False
    if dc is None:
        return not smp.data_consistency
    return (len(dc) == 2 and all(_rows_ok(t, y) and t.shape == deg.mask.shape and t.stride() == deg.mask.stride() for t in dc))


def supported(smp, y, blind):
    """True when this evaluation is a configuration babe_score_eval sequences (never for a network with time-attention layers:
    those run on the Python sequencer)."""
    m = smp.model
    return (y is not None and smp.norm == 2 and smp.stft_dist is None and smp.obs_snr is None and not smp.sigma_den
            and _observation_ok(smp, y, blind)
            and getattr(m, "precision", None) == "f32" and not getattr(m, "has_attention", False) and hasattr(m, "lane_engine") and cqt_plan_of(m.CQTransform) is not None)


class CEval:
    """One lane's descriptor + workspace (the UNet state and the workspace belong to one stream at a time)."""

    def __init__(self, smp, lane):
        from ..networks.unet_c import CUnet
        net, st = smp.model, smp._stft
        eng = net.lane_engine(lane or 0)
        # a library-side state of its own over the engine's plan: a score evaluation runs forward and VJP inside one call, and
        # may fall between a forward and the vjp of the engine state's own
        self.cu = CUnet(eng)
        cq = net.CQTransform
        self.cq_plan = cqt_plan_of(cq)
        d = EvalDesc()
        d.unet_plan, d.unet_state, d.cqt_plan, d.L = self.cu.plan, self.cu.state, self.cq_plan, cq.Ls
        d.rff_freq, d.rff_n = ptr(eng.rff_freq), eng.rff_freq.numel()
        d.emb_dim[0] = 2 * d.rff_n
        for i, (W, b) in enumerate(eng.emb_W):
            d.emb_W[i], d.emb_b[i], d.emb_dim[i + 1] = ptr(W), ptr(b), W.shape[0]
        d.film_W, d.film_b, d.film_J = ptr(eng.film_idx.Wcat), ptr(eng.film_idx.bcat), eng.film_idx.J
        d.nfft, d.fs, d.env_inv, d.tw4096 = st.nfft, st.fs, ptr(st.env_inv), ptr(st.tw4096)
        d.fit = smp.fit_cfg
        d.shared = int(smp.batch_semantics == "reference")
        d.hpf = int(bool(smp.args.tester.filter_out_cqt_DC_Nyq))
        d.xi, d.score_mode, d.audio_len_norm = float(smp.xi), int(smp.SCORE_MODE), float(smp.args.exp.audio_len)
        self.desc, self._ws = d, {}
        self._keep = (eng, st, cq)

    @staticmethod
    def observe(d, smp):
        """The observation model of the running call into descriptor d (all off without a degradation object)."""
        deg, dc = smp.degradation, smp.dc
        d.mask, d.mask_bs, d.dc_mask, d.dc_y = None, 0, None, None
        if deg is not None:
            m = deg.mask
            d.mask, d.mask_bs = ptr(m), (0 if m.dim() == 1 or m.shape[0] == 1 else m.stride(0))
            if dc is not None:
                d.dc_mask, d.dc_y = ptr(dc[0]), ptr(dc[1])

    def __call__(self, smp, x, t, y, specY, filter_params, blind):
        d = self.desc
        B, L = x.shape
        d.K, d.blind = int(filter_params.shape[-1]), int(bool(blind))
        self.observe(d, smp)
        ws = workspace(self._ws, B, lambda: lib().babe_eval_workspace_bytes(C.byref(d), B), x.device, "eval")
        dp = smp.diff_params
        s = torch.as_tensor(t, dtype=torch.float32)
        cskip, cout, cin, cnoise = float(dp.cskip(s)), float(dp.cout(s)), float(dp.cin(s)), float(dp.cnoise(s))
        p = filter_params.clone() if blind else filter_params.contiguous()
        dd, x_den = torch.empty_like(x), torch.empty_like(x)
        nit = torch.empty(p.shape[0], dtype=torch.int32, device=x.device)
        check(lib().babe_score_eval(C.byref(d), ptr(x), float(t), cskip, cout, cin, cnoise, ptr(y), ptr(specY), ptr(p), ptr(dd),
                                    ptr(x_den), ptr(nit), ptr(ws), ws.numel(), B, stream()), "score_eval")
        if blind:
            smp.last_n_iter = nit
        return dd, x_den, p
