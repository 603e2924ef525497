"""BlindSampler(loop="library"): a whole sampling run as ONE call into the library (csrc/sample.hip, babe_sample_bwe) - the path a
non-Python host takes: the evaluation descriptor of testing/eval_c.py, one babe_sample_step row per step made from the EDM object,
and the noise either as a [T+1][B][L] buffer or from the library's counter-based generator (csrc/randn.hip).  The
configurations of the library evaluation (predict_bwe_AR(..., 'fc_A') among them); everything else stays with the Python loop.
Bit-identical to it: tests/test_gpu_sample_c.py, tests/test_gpu_sample_ar_c.py."""
import ctypes as C

import torch

from .._cabi import SampleDesc, SampleStep
from .._lib import check, lib, ptr, stream, workspace
from . import eval_c


def supported(smp, y, blind, rid):
    """True when babe_sample_bwe runs this call: the library evaluation covers the configuration (eval_c.supported), the tensors
    are contiguous, and the records asked for are the ones it keeps (the blind loop's: the known-filter loop records the guided
    estimate and the score instead)."""
    return (eval_c.supported(smp, y, blind) and y.is_contiguous() and y.dtype == torch.float32 and (blind or not rid))


def precond(dp, t):
    """(cskip, cout, cin, cnoise) at noise level t (a host float), as BlindSampler.evaluate computes them."""
    s = torch.as_tensor(t, dtype=torch.float32)
    return float(dp.cskip(s)), float(dp.cout(s)), float(dp.cin(s)), float(dp.cnoise(s))


def steps_from(dp, T, order, start_sigma, snoise):
    """The step table of a run of T steps from the EDM object dp, with exactly the float expressions BlindSampler._inject and
    the Heun halves use -> (rows: a ctypes array of T babe_sample_step, t0, t: the schedule tensor [T + 1])."""
    t = dp.create_schedule(T) if start_sigma is None else dp.create_schedule_from_initial_t(start_sigma, T)
    gamma = dp.get_gamma(t)
    rows = (SampleStep * T)()
    for i in range(T):
        r = rows[i]
        t_hat = t[i] + gamma[i] * t[i]
        r.t_hat = float(t_hat)
        r.inject = float((t_hat ** 2 - t[i] ** 2) ** (1 / 2)) * float(snoise)
        r.t_next = float(t[i + 1])
        r.h = float(t[i + 1] - t_hat)
        r.heun = int(float(t[i + 1]) != 0 and order == 2)
        r.c1[:] = precond(dp, float(t_hat))
        if r.heun:
            r.c2[:] = precond(dp, float(t[i + 1]))
    return rows, float(t[0]), t


class CSample:
    """Descriptor and workspace of library-side runs on one stream at a time (the UNet state is that of its CEval)."""

    def __init__(self, smp, lane=None):
        self.ce = eval_c.CEval(smp, lane)
        self._ws = {}
        self.calls = 0                              # babe_sample_bwe calls made (tests/test_gpu_sample_c.py reads it)

    def __call__(self, smp, y, filter_params, blind, rows, t0, warm_start, noise=None, seed=0, clip0=0, rid=False):
        """y [B,L], filter_params [P,2,K] (left alone) -> (x, params) or, with rid, (x, params, rec_x_den [T,B,L], rec_params
        [T,P,2,K]), all on y's device.  noise: [T+1,B,L] on the device, or None for the generator under (seed, clip0)."""
        B, L = y.shape
        T = len(rows)
        d = SampleDesc()
        d.eval = self.ce.desc                       # (by value)
        d.eval.K, d.eval.blind = int(filter_params.shape[-1]), int(bool(blind))
        eval_c.CEval.observe(d.eval, smp)
        d.T, d.steps, d.t0, d.warm_start = T, rows, t0, int(bool(warm_start))
        ws = workspace(self._ws, (B, T), lambda: lib().babe_sample_workspace_bytes(C.byref(d), B), y.device, "sample")
        if noise is not None:
            assert noise.shape == (T + 1, B, L) and noise.is_contiguous() and noise.dtype == torch.float32 and noise.device == y.device
        p = filter_params.clone().contiguous()
        x = torch.empty_like(y)
        rec_x = torch.empty((T, B, L), device=y.device) if rid else None
        rec_p = torch.empty((T, *p.shape), device=y.device) if rid else None
        self.calls += 1
        check(lib().babe_sample_bwe(C.byref(d), ptr(y), ptr(p), ptr(x), ptr(noise), int(seed), int(clip0), ptr(rec_x), ptr(rec_p),
                                    ptr(ws), ws.numel(), B, stream()), "sample_bwe")
        return (x, p, rec_x, rec_p) if rid else (x, p)
