"""Karras-EDM parameterisation, host side.  Same surface as /root/reference/diff_params/edm.py
(EDM :7-159): create_schedule :55-64, create_schedule_from_initial_t :66-75, get_gamma :38-53,
sample_prior :98-106, cskip/cout/cin/cnoise :108-139, denoiser :144-159, mutable sigma_* / S* fields
(mutated by BlindSampler.update_diff_params, blind_bwe_sampler.py:50-60).  Scalars stay float32
torch CPU tensors so schedules are bit-identical to the reference; tensors on the GPU go through
the babe_hip element-wise kernel."""
import torch

from ..stft import fir_sqerr, lincomb
from ..utils.training_utils import FIRFilter


class EDM:
    def __init__(self, args):
        self.args = args
        dp = args.diff_params
        self.sigma_min, self.sigma_max = dp.sigma_min, dp.sigma_max
        self.P_mean, self.P_std = dp.get("P_mean", -1.2), dp.get("P_std", 1.2)
        self.ro, self.ro_train = dp.ro, dp.get("ro_train", dp.ro)
        self.sigma_data = dp.sigma_data
        self.Schurn, self.Stmin, self.Stmax, self.Snoise = dp.Schurn, dp.Stmin, dp.Stmax, dp.Snoise
        self.AW = None                                   # perceptual weighting of the training error (edm.py:33-34)
        aw = dp.get("aweighting", None) or {}
        if aw.get("use_aweighting", False):
            self.AW = FIRFilter(filter_type="aw", fs=args.exp.sample_rate, ntaps=aw.get("ntaps", 101))

    def get_gamma(self, t):
        N = t.shape[0]
        gamma = torch.zeros(t.shape)
        sel = torch.logical_and(t > self.Stmin, t < self.Stmax)
        gamma[sel] = gamma[sel] + torch.min(torch.Tensor([self.Schurn / N, 2 ** (1 / 2) - 1]))
        return gamma

    def _sched(self, s0, nb_steps):
        i = torch.arange(0, nb_steps + 1)
        t = (s0 ** (1 / self.ro) + i / (nb_steps - 1) * (self.sigma_min ** (1 / self.ro) - s0 ** (1 / self.ro))) ** self.ro
        t[-1] = 0
        return t

    def create_schedule(self, nb_steps):
        return self._sched(self.sigma_max, nb_steps)

    def create_schedule_from_initial_t(self, initial_t, nb_steps):
        return self._sched(initial_t, nb_steps)

    def sample_prior(self, shape, sigma):
        return torch.randn(shape) * sigma

    # ---------------------------------------------------------------- training (reference edm.py:88-96, :161-206)
    def sample_ptrain_safe(self, N):
        """N training noise levels drawn like the sampling schedule: torch.rand(N) on the CPU generator."""
        a = torch.rand(N)
        return (self.sigma_max ** (1 / self.ro_train) + a * (self.sigma_min ** (1 / self.ro_train) -
                                                              self.sigma_max ** (1 / self.ro_train))) ** self.ro_train

    def prepare_train_preconditioning(self, x, sigma):
        """(cin*(x+n), (x - cskip*(x+n))/cout, cnoise) with n = randn(x.shape) * sigma drawn on the CPU generator (as the
        reference's sample_prior) and moved to x's device."""
        noise = torch.randn(x.shape).to(sigma.device) * sigma
        cskip, cout, cin, cnoise = self.cskip(sigma), self.cout(sigma), self.cin(sigma), self.cnoise(sigma)
        target = (1 / cout) * (x - cskip * (x + noise))
        return cin * (x + noise), target, cnoise

    def loss_fn(self, net, x, return_residual=False):
        """(error**2 [B,L], sigma [B,1]) of the denoising objective for clean audio x [B,L]: draws sigma (torch.rand) then the
        noise (torch.randn), like the reference.  The reference's DC correction reads args.net.use_cqt_DC_correction - a key no
        configuration defines (they have exp.use_cqt_DC_correction) - inside a bare except, so it never runs; it is left out
        here for the same result.  With diff_params.aweighting.use_aweighting the error goes through the A-weighting FIR before
        the square (edm.py:201-203): subtraction, filter and square are one HIP kernel (stft.fir_sqerr), and so is their backward;
        without it the tail is the two torch operations below, as before.
        return_residual: also return the signed error before the square (the A-weighted one where that is on), detached - what
        the training log's loss-by-frequency transforms (training.Trainer); the other two results are the same tensors either way."""
        sigma = self.sample_ptrain_safe(x.shape[0]).unsqueeze(-1).to(x.device)
        inp, target, cnoise = self.prepare_train_preconditioning(x, sigma)
        estimate = net(inp, cnoise)
        if self.AW is not None:
            err2, ew = fir_sqerr(estimate, target, self.AW.to(estimate.device).taps, return_filtered=True)
            return (err2, sigma, ew) if return_residual else (err2, sigma)
        error = estimate - target
        return (error ** 2, sigma, error.detach()) if return_residual else (error ** 2, sigma)

    def cskip(self, sigma):
        return self.sigma_data ** 2 * (sigma ** 2 + self.sigma_data ** 2) ** -1

    def cout(self, sigma):
        return sigma * self.sigma_data * (self.sigma_data ** 2 + sigma ** 2) ** (-0.5)

    def cin(self, sigma):
        return (self.sigma_data ** 2 + sigma ** 2) ** (-0.5)

    def cnoise(self, sigma):
        return (1 / 4) * torch.log(torch.as_tensor(sigma, dtype=torch.float32))

    def denoiser(self, xn, net, sigma):
        """cskip*x + cout*net(cin*x, cnoise) for ONE sigma shared by the batch (like the reference's use)."""
        s = torch.as_tensor(sigma, dtype=torch.float32).reshape(-1)[0].cpu()
        B = xn.shape[0]
        xin = lincomb(torch.empty_like(xn), float(self.cin(s)), xn.contiguous())
        cn = self.cnoise(s).reshape(1, 1).expand(B, 1).contiguous().to(xn.device)
        out = net(xin, cn)
        return lincomb(torch.empty_like(xn), float(self.cskip(s)), xn.contiguous(), float(self.cout(s)), out.contiguous())
