"""Known-degradation EDM sampler (config #1) on the babe_hip kernels.

Drop-in for the reference's ``testing.edm_sampler.Sampler`` (/root/reference/testing/edm_sampler.py:8-305):
``Sampler(model, diff_params, args, rid=False)``, ``predict_bwe(ylpf, filt, 'firwin')`` :266-305 ->
``predict_conditional`` -> ``predict`` :166-229 with ``get_score_rec_guidance`` :56-94.  Differences from
BlindSampler that matter for parity: the schedule always starts from sigma_max with a pure
prior sample (:177-179); no noise is drawn on steps with gamma == 0 (:187-198); Snoise scales the noise;
the guidance scale is xi/(||g||/sqrt(L)*t + 1e-6) without the extra 1/t (:78-92).
Only the FIR degradation ('firwin' / 'firwin_hpf') runs on the HIP path; IIR/biquad/resample/decimate
are torchaudio paths that no target config uses.

Declipping, compressed sensing and phase retrieval (:308-384) are the same loop with another observation operator:
predict_declipping, predict_compsens, predict_pr.  The reference's own SamplerDeclipping / SamplerCompSens /
SamplerPhaseRetrieval cannot be constructed (they hand seven arguments to this class's four-argument constructor and read an
``args.inference`` no YAML defines), so the entry points live here, on the base class the reference's fixtures come from.
"""
import torch

from ..degrade import ClipDegradation, FIRDegradation, MaskDegradation, STFTMagnitudeDegradation
from ..stft import STFTOps, lincomb
from .blind_bwe_sampler import BlindSampler


class Sampler(BlindSampler):
    SCORE_MODE = 1

    def __init__(self, model, diff_params, args, rid=False, batch_semantics="per_clip", noise_device="cpu"):
        # posterior_sampling.data_consistency (:47-54, :113-122): after the guided score, the replacement step
        # x0 <- y + x0 - A(x0) on the Tweedie estimate - BlindSampler.evaluate's classic branch with the FIR as A.
        # xi = 0 (:124-130): no guidance at all, the replacement step on the plain denoised estimate (evaluate below).
        self._init_common(model, diff_params, args, batch_semantics, noise_device)
        self.rid = rid
        self.norm, self.smoothl1_beta, self.stft_dist = 2, 1.0, None      # edm_sampler.py:71: torch.linalg.norm(y - den_rec, ord=2) only

    def stft_ops(self, L, device):
        if self._stft is None or self._stft.L != L:
            self._stft = STFTOps(4096, L, self.args.exp.sample_rate, device)     # only its residual_seed helper is used
        return self._stft

    def evaluate(self, x, t, y, specY, filter_params, blind, lane=None):
        if self.xi > 0 or y is None:
            return super().evaluate(x, t, y, specY, filter_params, blind, lane)
        # xi = 0: x0 = D(x) (no high-pass in this branch of the reference, :126), x0 <- y + x0 - A(x0), d = (x - x0) / t
        x_den = self.get_denoised_estimate(x, t, lane, hpf=False)
        x0 = lincomb(torch.empty_like(x), 1.0, x_den, 1.0, y, -1.0, self.degradation.fwd_dc(x_den))
        return lincomb(torch.empty_like(x), 1.0 / float(t), x, -1.0 / float(t), x0), x_den, filter_params

    def predict_bwe(self, ylpf, filt, filt_type):
        if filt_type not in ("firwin", "firwin_hpf"):
            raise NotImplementedError(f"filt_type={filt_type!r}: only FIR degradations run on the HIP path")
        with self._guiding(FIRDegradation(filt, ylpf.device)):
            return self.predict_conditional(ylpf)

    def predict_inpainting(self, y_masked, mask):
        """Masking degradation A(x) = mask * x (edm_sampler.py:231-243 -> predict_conditional): y_masked [B,L], mask [L] or [B,L]
        (1 = observed).  Guidance gradient through the mask, data-consistency replacement x0 <- y + x0 - mask * x0 if configured."""
        with self._guiding(MaskDegradation(mask, y_masked.device)):
            return self.predict_conditional(y_masked)

    def _require_guidance(self, what, allow_dc=False):
        """The rules the reference's task subclasses assert (:314-315, :340-341, :366): guidance on, no replacement step."""
        if not self.xi > 0:
            raise ValueError(f"{what}: posterior_sampling.xi must be > 0 (reconstruction guidance is the only way this "
                             f"observation enters), got {self.xi}")
        if self.data_consistency and not allow_dc:
            raise ValueError(f"{what}: posterior_sampling.data_consistency must be False (the replacement step "
                             f"x0 <- y + x0 - A(x0) holds for linear A only)")

    def predict_declipping(self, y_clipped, clip_value):
        """Declipping (SamplerDeclipping :308-332): A(x) = clip(x, -clip_value, clip_value), y_clipped [B,L] on the GPU.
        Needs xi > 0 and data_consistency off."""
        self._require_guidance("predict_declipping")
        with self._guiding(ClipDegradation(clip_value)):
            return self.predict_conditional(y_clipped)

    def predict_compsens(self, y_masked, mask):
        """Compressed sensing (SamplerCompSens :334-357): A(x) = mask * x with a random 0/1 mask [L] or [B,L] - the operator of
        predict_inpainting, under the rules of the reference's subclass: xi > 0, data_consistency off."""
        self._require_guidance("predict_compsens")
        with self._guiding(MaskDegradation(mask, y_masked.device)):
            return self.predict_conditional(y_masked)

    def predict_pr(self, y, win_size=None, hop_size=None):
        """Phase retrieval (SamplerPhaseRetrieval :359-384): y = |STFT(cat(x, zeros(win)))| with a periodic Hamming window,
        center=False, as [B, win/2+1, frames] or flattened [B, (win/2+1) frames]; the state has shape (B, args.exp.audio_len).
        win_size / hop_size default to tester.phase_retrieval.win_size / hop_size (1024 / 256 where the YAML has no such key).
        Needs xi > 0; with data_consistency the reference calls a step it never defines: NotImplementedError.  The gradient of
        the magnitude at a bin that is exactly zero is taken as 0 (degrade.STFTMagnitudeDegradation).
        The guidance distance is the reference's: torch.linalg.norm(y - A(x), dim=(1, 2), ord=2) on its 3-D observation is
        the MATRIX 2-norm, the largest singular value of the bins x frames residual (degrade.specnorm_seed), not the vector
        norm of the other tasks - whichever layout y arrives in."""
        self._require_guidance("predict_pr", allow_dc=True)
        if self.data_consistency:
            raise NotImplementedError("predict_pr: posterior_sampling.data_consistency has no step to run (the reference calls "
                                      "data_consistency_step_phase_retrieval, which is defined nowhere)")
        pr = self.args.tester.get("phase_retrieval", None) or {}
        win = int(win_size if win_size is not None else pr.get("win_size", 1024))
        hop = int(hop_size if hop_size is not None else pr.get("hop_size", 256))
        L = int(self.args.exp.audio_len)
        deg = STFTMagnitudeDegradation(win, hop, L, y.device, matrix_norm=True)
        B = y.shape[0]
        if tuple(y.shape[1:]) not in (deg.out_shape(), (deg.bins * deg.frames,)):
            raise ValueError(f"predict_pr: y has shape {tuple(y.shape)}, the degradation of audio_len = {L} yields "
                             f"(B, {deg.bins}, {deg.frames})")
        with self._guiding(deg):
            return self.predict_conditional(y.reshape(B, -1), shape=(B, L))

    def predict_unconditional(self, shape, device):
        """Unguided sampling (edm_sampler.py:231-243 -> predict :166-229 with y = None)."""
        return self.predict_conditional(None, shape=tuple(shape), device=torch.device(device))

    def predict_conditional(self, y, shape=None, device=None):
        dp = self.diff_params
        if y is not None:
            y = y.contiguous().float()
            shape, device = (y.shape if shape is None else tuple(shape)), y.device      # (predict_pr: y is not a signal)
        B, L = shape
        self.stft_ops(L, device)
        T = self.nb_steps
        if self.rid:
            data_denoised = torch.zeros((T, B, L))
        t = dp.create_schedule(T)
        s = dict(x=(self._randn((B, L), device) * float(t[0])).contiguous(), fp=None)
        gamma = dp.get_gamma(t)
        ev = lambda x_, t_, fp: self.evaluate(x_, t_, y, None, fp, blind=False)
        for i in range(T):
            # no noise is drawn on a step with gamma == 0 (:187-198): the state is evaluated as it is
            eps = self._randn((B, L), device).contiguous() if float(gamma[i]) != 0 else None
            self._heun_first(s, t[i], gamma[i], t[i + 1], eps, dp.Snoise, ev)
            self._heun_second(s, t[i + 1], ev)
            if self.rid:
                data_denoised[i] = s["x"].cpu()
        return (s["x"], data_denoised, t) if self.rid else s["x"]
