"""The library-side workspaces are sized by the carve that uses them (csrc/workspace.h): babe_score_eval and babe_sample_bwe run in
exactly babe_*_workspace_bytes bytes and leave what lies behind them alone, one byte less is refused on the host, and the CQT
plan's size is the three buffers of the numpy design.  Fixture of tests/test_gpu_eval_c.py; odd B, and P = 1 < B (the reference's
batch coupling), are where the small pieces round differently.  Needs a MI355X."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

NS, L, FS = [8, 8, 8, 8, 16, 16, 16], 92092, 22050
CASES = [(1, "per_clip"), (3, "per_clip"), (2, "reference")]
TAIL = 4096


@pytest.fixture(scope="module")
def world():
    """One network and one set of observations for the whole file (never modified)."""
    from babe_amd.config import default_args
    from babe_amd.networks.cqtdiff_plus import Unet_CQT_oct_with_attention, init_state_dict
    mp = pytest.MonkeyPatch()
    mp.setenv("BABE_CQT_C", "1")
    args = default_args(sample_rate=FS, audio_len=L, Ns=NS, T=2, start_sigma=0.05)
    net = Unet_CQT_oct_with_attention(args, "cuda")
    net.load_state_dict(init_state_dict(NS, args.network.num_dils, seed=0, gate_scale=1.0))
    g = torch.Generator().manual_seed(5)
    y = (0.1 * torch.randn(3, L, generator=g)).cuda()
    x = (y.cpu() + 0.05 * torch.randn(3, L, generator=g)).cuda()
    yield dict(args=args, net=net, y=y, x=x)
    mp.undo()


def _sampler(world, B, semantics):
    """-> (sampler, y [B,L], x [B,L], specY, filter parameters [P,2,K])"""
    from babe_amd.diff_params.edm import EDM
    from babe_amd.testing.blind_bwe_sampler import BlindSampler
    smp = BlindSampler(world["net"], EDM(world["args"]), world["args"], batch_semantics=semantics)
    y, x = world["y"][:B].contiguous(), world["x"][:B].contiguous()
    specY = smp.stft_ops(L, y.device).stft(y)
    ic = smp.args.tester.blind_bwe.initial_conditions
    P = 1 if semantics == "reference" else B
    fp = torch.tensor([list(ic.fc), list(ic.A)], dtype=torch.float32).unsqueeze(0).repeat(P, 1, 1).cuda()
    return smp, y, x, specY, fp


def _check_exact(need, run, outputs):
    """run(buffer, declared bytes) -> (status, output tensors): the three checks both entry points get."""
    from babe_amd._lib import dispatch_counts, lib
    assert need > 0 and need % 256 == 0
    buf = torch.empty(need + TAIL, device="cuda", dtype=torch.uint8)
    pattern = (torch.arange(TAIL, device="cuda") % 251 + 1).to(torch.uint8)
    buf[need:] = pattern
    rc, exact = run(buf, need)
    torch.cuda.synchronize()
    assert rc == 0, lib().babe_last_error()
    assert torch.equal(buf[need:], pattern), "the call wrote behind the bytes it asked for"
    rc, whole = run(buf, need + TAIL)
    torch.cuda.synchronize()
    assert rc == 0, lib().babe_last_error()
    assert len(exact) == outputs and all(torch.isfinite(u).all() and torch.equal(u, v) for u, v in zip(exact, whole))
    launches = dispatch_counts()
    rc, _ = run(buf, need - 1)
    msg = lib().babe_last_error().decode()
    assert rc < 0 and f"workspace of {need - 1} bytes, need {need}" in msg, (rc, msg)
    assert dispatch_counts() == launches, "a refused call launched"


@pytest.mark.parametrize("B,semantics", CASES)
def test_score_eval_runs_in_exactly_the_bytes_it_asks_for(world, B, semantics):
    from babe_amd._lib import lib, ptr, stream
    from babe_amd.testing import eval_c, sample_c
    smp, y, x, specY, fp = _sampler(world, B, semantics)
    ce = eval_c.CEval(smp, 0)                                  # (owns the UNet state the descriptor points to)
    d = ce.desc
    d.K, d.blind = fp.shape[-1], 1
    t = 0.05
    c = sample_c.precond(smp.diff_params, t)

    def run(buf, nbytes):
        p, dd, x_den = fp.clone(), torch.zeros_like(x), torch.zeros_like(x)
        rc = lib().babe_score_eval(C.byref(d), ptr(x), t, *c, ptr(y), ptr(specY), ptr(p), ptr(dd), ptr(x_den), None, ptr(buf), nbytes, B,
                                   stream())
        return rc, (dd, x_den, p)
    _check_exact(lib().babe_eval_workspace_bytes(C.byref(d), B), run, 3)


@pytest.mark.parametrize("B,semantics", CASES)
def test_sample_bwe_runs_in_exactly_the_bytes_it_asks_for(world, B, semantics):
    """T = 2: one Heun step and the final Euler step, noise from the library's generator."""
    from babe_amd._cabi import SampleDesc
    from babe_amd._lib import lib, ptr, stream
    from babe_amd.testing import eval_c, sample_c
    smp, y, x, specY, fp = _sampler(world, B, semantics)
    rows, t0, _ = sample_c.steps_from(smp.diff_params, 2, smp.order, smp.start_sigma, 1.0)
    assert [r.heun for r in rows] == [1, 0]
    ce = eval_c.CEval(smp, 0)
    d = SampleDesc()
    d.eval = ce.desc
    d.eval.K, d.eval.blind = fp.shape[-1], 1
    d.T, d.steps, d.t0, d.warm_start = 2, rows, t0, 1

    def run(buf, nbytes):
        p, out = fp.clone(), torch.zeros_like(y)
        rc = lib().babe_sample_bwe(C.byref(d), ptr(y), ptr(p), ptr(out), None, 7, 0, None, None, ptr(buf), nbytes, B, stream())
        return rc, (out, p)
    need = lib().babe_sample_workspace_bytes(C.byref(d), B)
    assert need > lib().babe_eval_workspace_bytes(C.byref(d.eval), B)
    _check_exact(need, run, 2)


def test_cqt_workspace_is_the_three_buffers_of_the_numpy_design(world):
    from babe_amd._lib import lib
    cq = world["net"].CQTransform
    assert cq._plan
    for B in (1, 2, 3):
        assert lib().babe_cqt_workspace_bytes(cq._plan, B) == 8 * B * (cq.fft.KX + cq.Ls + cq.nwin) + 1024
