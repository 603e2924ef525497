"""Known degradations and the EDM sampler's tasks on the library path: babe_score_eval with desc.obs_kind / dc_classic / y = NULL
against the Python sequencers (BlindSampler.evaluate, score_mode 0; edm_sampler.Sampler.evaluate, score_mode 1), whole
babe_sample_bwe runs against BlindSampler.predict_bwe / predict_bwe_AR and the Sampler's tasks, the seeded run, the exact
workspace and the C host's --fir option.  Both sides launch the same kernels on the same data in the same order, so every
comparison is torch.equal.  Reduced network and fixture shape of tests/test_gpu_sample_c.py.  Needs a MI355X."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NS, L, FS, T = [8, 8, 8, 8, 16, 16, 16], 92092, 22050, 3
T_EVAL = float(torch.tensor(0.05, dtype=torch.float32))       # a noise level that is a float32, as every level of a schedule is


def _args():
    from babe_amd.config import default_args
    return default_args(sample_rate=FS, audio_len=L, Ns=NS, T=T, start_sigma=0.05)


class _World:
    """One network, its library-side descriptor, observations and T + 1 noise tensors for the whole file (never modified)."""

    def __init__(self, tmp):
        from babe_amd.diff_params.edm import EDM
        from babe_amd.networks.cqtdiff_plus import Unet_CQT_oct_with_attention, init_state_dict
        from babe_amd.testing import eval_c
        from babe_amd.testing.blind_bwe_sampler import BlindSampler
        self.tmp = str(tmp)
        args = _args()
        self.sd = init_state_dict(NS, args.network.num_dils, seed=0, gate_scale=1.0)
        self.net = Unet_CQT_oct_with_attention(args, "cuda")
        self.net.load_state_dict(self.sd)
        g = torch.Generator().manual_seed(5)
        self.y = (0.1 * torch.randn(2, L, generator=g)).cuda()
        self.noises = [torch.randn(2, L, generator=g) for _ in range(T + 1)]
        self.mask_row = (torch.rand(L, generator=g) < 0.6).float().cuda()                # [L]
        self.mask_rows = (torch.rand(2, L, generator=g) < 0.6).float().cuda()            # [B][L]
        self.ar_mask = torch.zeros(2, L)
        self.ar_mask[0, :5512] = 1
        self.ar_mask[1, :9000] = 1
        self.ar_mask = self.ar_mask.cuda()
        # the descriptor of the network, from the Python engine (testing/eval_c.py); the tests copy it and set the sampler's scalars
        self.owner = BlindSampler(self.net, EDM(args), args)
        self.owner.stft_ops(L, "cuda")
        self.ce = eval_c.CEval(self.owner, None)
        self._model = None

    def desc(self, smp, semantics):
        from babe_amd._cabi import EvalDesc
        d = EvalDesc.from_buffer_copy(self.ce.desc)
        d.K, d.blind, d.shared = 1, 0, int(semantics == "reference")
        d.xi, d.score_mode, d.hpf = float(smp.xi), int(smp.SCORE_MODE), int(bool(smp.args.tester.filter_out_cqt_DC_Nyq))
        d.mask, d.mask_bs, d.dc_mask, d.dc_y = None, 0, None, None
        return d

    def model(self):
        from babe_amd import model_file
        from babe_amd.testing.model_c import LibraryModel
        if self._model is None:
            self.path = os.path.join(self.tmp, "small.babe")
            model_file.export(self.sd, _args(), self.path)
            self._model = LibraryModel(self.path)
        return self._model

    def close(self):
        if self._model is not None:
            self._model.close()


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    mp = pytest.MonkeyPatch()
    mp.setenv("BABE_CQT_C", "1")                       # the Python sequencer on the library's CQT plan (same tables)
    import babe_amd.testing.blind_bwe_sampler as bs
    mp.setattr(bs, "EVAL_C", False)                    # ... and sequencing every evaluation itself
    w = _World(tmp_path_factory.mktemp("obs"))
    yield w
    w.close()
    mp.undo()


def _sampler(world, mode, semantics="per_clip", xi=None, dc=False, **kw):
    """mode 0: BlindSampler, mode 1: edm_sampler.Sampler, on the one network."""
    from babe_amd.diff_params.edm import EDM
    from babe_amd.testing.blind_bwe_sampler import BlindSampler
    from babe_amd.testing.edm_sampler import Sampler
    args = _args()
    if xi is not None:
        args.tester.posterior_sampling.xi = xi
    args.tester.posterior_sampling.data_consistency = bool(dc)
    smp = (Sampler if mode else BlindSampler)(world.net, EDM(args), args, batch_semantics=semantics, **kw)
    smp.stft_ops(L, "cuda")
    return smp


def _fir_taps(numtaps):
    from babe_amd.testing import model_c
    return torch.as_tensor(model_c.firwin_kaiser(numtaps, 2000, 300, FS), dtype=torch.float32)


def _cheby1():
    from babe_amd.utils.bandwidth_extension import get_cheby1_ba
    return get_cheby1_ba(6, 0.05, 2 * 3000 / FS)


def _biquad():
    from babe_amd.utils.bandwidth_extension import design_biquad_lpf
    return design_biquad_lpf(3000, FS, 0.707)


# name -> (degradation factory (world, B), scale of y, dc_classic, xi override, score modes)
def _cases():
    from babe_amd import degrade as dg
    dev = "cuda"
    fir = lambda n: (lambda w, B: dg.FIRDegradation(_fir_taps(n), dev))
    return {
        "fir33": (fir(33), 1.0, False, None, (0, 1)),
        "fir32": (fir(32), 1.0, False, None, (0, 1)),
        "cheby1": (lambda w, B: dg.make_degradation(_cheby1(), "cheby1", dev)[0], 1.0, False, None, (0, 1)),
        "biquad": (lambda w, B: dg.make_degradation(_biquad(), "biquad", dev)[0], 20.0, False, None, (0, 1)),
        "mask_L": (lambda w, B: dg.MaskDegradation(w.mask_row, dev), 1.0, False, None, (0, 1)),
        "mask_BL": (lambda w, B: dg.MaskDegradation(w.mask_rows[:B].contiguous(), dev), 1.0, False, None, (0, 1)),
        "clip": (lambda w, B: dg.ClipDegradation(0.05), 1.0, False, None, (0, 1)),
        "ar_fir": (lambda w, B: dg.MaskMixDegradation(w.ar_mask[:B].contiguous(), dg.FIRDegradation(_fir_taps(33), dev)), 1.0, False,
                   None, (0, 1)),
        "dc_fir": (fir(33), 1.0, True, None, (0, 1)),
        "dc_mask": (lambda w, B: dg.MaskDegradation(w.mask_row, dev), 1.0, True, None, (0, 1)),
        "xi0_fir": (fir(33), 1.0, True, 0.0, (1,)),
        "xi0_mask": (lambda w, B: dg.MaskDegradation(w.mask_rows[:B].contiguous(), dev), 1.0, True, 0.0, (1,)),
        "no_y": (None, 1.0, False, None, (0, 1)),
    }


def _counted(run):
    from babe_amd._lib import dispatch_counts
    torch.cuda.synchronize()
    dispatch_counts(reset=True)
    res = run()
    torch.cuda.synchronize()
    return res, {k: v for k, v in dispatch_counts(reset=True).items() if v}


def _lib_eval(d, dp, x, t, y):
    from babe_amd._lib import check, lib, ptr, stream
    from babe_amd.testing import sample_c
    B = x.shape[0]
    n = lib().babe_eval_workspace_bytes(C.byref(d), B)
    assert n > 0, lib().babe_last_error()
    ws = torch.empty(n, dtype=torch.uint8, device="cuda")
    dd, x_den = torch.empty_like(x), torch.empty_like(x)
    check(lib().babe_score_eval(C.byref(d), ptr(x), t, *sample_c.precond(dp, t), ptr(y), None, None, ptr(dd), ptr(x_den), None, ptr(ws),
                                n, B, stream()), "score_eval")
    torch.cuda.synchronize()
    return dd, x_den


@pytest.mark.parametrize("name", ["fir33", "fir32", "cheby1", "biquad", "mask_L", "mask_BL", "clip", "ar_fir", "dc_fir", "dc_mask",
                                  "xi0_fir", "xi0_mask", "no_y"])
def test_one_evaluation_equals_the_python_sequencer_bit_for_bit(world, name):
    """babe_score_eval = BlindSampler.evaluate (score_mode 0) / edm_sampler.Sampler.evaluate (score_mode 1) sequencing the kernels
    itself, in d and x_den: B = 1, and B = 2 with per-clip and with the reference's batch semantics.  The launch counters of the
    two sides agree slot by slot - at B = 2 outside the UNet's layers - (printed: the launches per evaluation of this kind)."""
    from babe_amd.stft import lincomb
    from babe_amd.testing import model_c
    make, yscale, dc, xi, modes = _cases()[name]
    for mode in modes:
        for B, semantics in ((1, "per_clip"), (2, "per_clip"), (2, "reference")):
            smp = _sampler(world, mode, semantics, xi=xi, dc=dc)
            deg = make(world, B) if make else None
            y = None
            x = lincomb(torch.empty(B, L, device="cuda"), T_EVAL, world.noises[0][:B].contiguous().cuda())
            if make:
                y = (yscale * world.y[:B]).contiguous()
                if name == "clip":
                    y = torch.clip(y, -deg.c, deg.c)
                x = lincomb(torch.empty_like(y), 1.0, y, 1.0, x)

            def python():
                with smp._guiding(deg):
                    d, x_den, _ = smp.evaluate(x, T_EVAL, y, None, None, False)
                return d.clone(), x_den.clone()

            (d_py, xd_py), n_py = _counted(python)
            desc = model_c.observe(world.desc(smp, semantics), deg, dc_classic=dc)
            (d_c, xd_c), n_c = _counted(lambda: _lib_eval(desc, smp.diff_params, x, T_EVAL, y))
            if (mode, B) == (modes[0], 1):
                print(f"{name}: launches per evaluation: python {sum(n_py.values())}, library {sum(n_c.values())}: {n_c}")
            assert torch.isfinite(d_c).all() and torch.isfinite(xd_c).all() and d_c.abs().max() > 0
            assert torch.equal(xd_c, xd_py), (name, mode, B, semantics, float((xd_c - xd_py).abs().max()))
            assert torch.equal(d_c, d_py), (name, mode, B, semantics, float((d_c - d_py).abs().max()))
            if B > 1:                                  # (the Python engine runs some UNet layers clip by clip, the C sequencer
                net = ("conv", "gn_", "scale_gelu", "resample", "axpby")             # batches them: those slots count differently)
                n_c, n_py = ({k: v for k, v in n.items() if not k.startswith(net)} for n in (n_c, n_py))
            assert n_c == n_py, (name, mode, B, semantics, n_c, n_py)
            if name in ("biquad", "clip"):             # both regions of the mask occur (the Python object keeps the forward's)
                m = deg.mask
                assert m.dtype == torch.uint8 and int(m.min()) == 0 and int(m.max()) == 1, name


# ------------------------------------------------------------------------------------------------------------- whole runs
def _feed(smp, noises, B):
    it = iter(noises)
    smp._randn = lambda shape, device: next(it)[:B].contiguous().to(device)


def _noise_buffer(world, B):
    return torch.stack([n[:B] for n in world.noises]).contiguous().cuda()


def _lib_run(desc, y, rows, t0, warm, noise=None, seed=0, clip0=0, skip=False, shape=None):
    from babe_amd.testing import model_c
    x, _, _ = model_c.sample(None, None, y, None, rows, t0, warm, seed, clip0=clip0, blind=False, desc=desc, noise=noise,
                             skip_zero_inject=skip, shape=shape)
    assert torch.isfinite(x).all()
    return x


@pytest.mark.parametrize("filt_type,B", [("firwin", 1), ("firwin", 2), ("cheby1", 2), ("biquad", 2)])
def test_predict_bwe_with_a_known_degradation_equals_the_library_run(world, filt_type, B):
    """babe_sample_bwe on a noise buffer = BlindSampler.predict_bwe(y, filt, 'firwin' | 'cheby1' | 'biquad') fed the same tensors."""
    from babe_amd.degrade import make_degradation
    from babe_amd.testing import model_c, sample_c
    filt = {"firwin": lambda: _fir_taps(33), "cheby1": _cheby1, "biquad": _biquad}[filt_type]()
    y = world.y[:B].contiguous()
    smp = _sampler(world, 0)
    _feed(smp, world.noises, B)
    want = smp.predict_bwe(y, filt, filt_type)
    torch.cuda.synchronize()
    dp = smp.diff_params
    rows, t0, _ = sample_c.steps_from(dp, T, smp.order, smp.start_sigma, dp.Snoise)
    desc = model_c.observe(world.desc(smp, "per_clip"), make_degradation(filt, filt_type, "cuda", L)[0])
    got = _lib_run(desc, y, rows, t0, True, _noise_buffer(world, B))
    assert torch.equal(got, want), float((got - want).abs().max())


def test_predict_bwe_AR_over_a_fir_equals_the_library_run(world):
    """predict_bwe_AR(..., 'firwin') with the inpaint_DC pair: the AR mix over the FIR (desc.mask with BABE_OBS_FIR) and the
    replacement step of desc.dc_mask / dc_y."""
    from babe_amd._lib import ptr
    from babe_amd.degrade import FIRDegradation, MaskMixDegradation
    from babe_amd.stft import mask_blend
    from babe_amd.testing import model_c, sample_c
    ylpf, mask = world.y[:1].contiguous(), world.ar_mask[:1].contiguous()
    y_masked = (mask * world.y[1:2]).contiguous()
    smp = _sampler(world, 0)
    assert smp.args.tester.complete_recording.inpaint_DC
    _feed(smp, world.noises, 1)
    want = smp.predict_bwe_AR(ylpf, y_masked, _fir_taps(33), "firwin", mask=mask)
    torch.cuda.synchronize()
    dp = smp.diff_params
    rows, t0, _ = sample_c.steps_from(dp, T, smp.order, smp.start_sigma, dp.Snoise)
    desc = model_c.observe(world.desc(smp, "per_clip"), MaskMixDegradation(mask, FIRDegradation(_fir_taps(33), "cuda")))
    sm = smp.prepare_smooth_mask(mask, 50)
    y_sm = mask_blend(sm, y_masked, None)
    desc.dc_mask, desc.dc_y = ptr(sm), ptr(y_sm)
    got = _lib_run(desc, mask_blend(mask, y_masked, ylpf), rows, t0, True, _noise_buffer(world, 1))
    assert torch.equal(got, want), float((got - want).abs().max())


def _edm_sampler(world, **kw):
    """An edm_sampler.Sampler whose schedule has a step without churn and steps with it: Stmax between the first two levels."""
    smp = _sampler(world, 1, **kw)
    dp = smp.diff_params
    t = dp.create_schedule(T)
    dp.Stmin, dp.Stmax = 0.0, float((t[0] + t[1]) / 2)
    gamma = dp.get_gamma(t)
    assert float(gamma[0]) == 0 and float(gamma[1]) > 0 and float(gamma[2]) > 0
    return smp, gamma


def _feed_edm(smp, world, gamma, B):
    """Row 0 is the initial state, row i + 1 belongs to step i whether or not the step draws: the Python loop, which draws only
    where gamma != 0, is fed exactly those rows."""
    _feed(smp, [world.noises[0]] + [world.noises[i + 1] for i in range(T) if float(gamma[i]) != 0], B)


@pytest.mark.parametrize("task", ["bwe", "inpainting", "compsens", "declipping", "unconditional", "bwe_dc"])
def test_edm_sampler_tasks_equal_the_library_run(world, task):
    """babe_sample_bwe with skip_zero_inject = edm_sampler.Sampler.predict_bwe('firwin') / predict_inpainting / predict_compsens /
    predict_declipping / predict_unconditional in the final x (B = 2), on a schedule whose gamma has zero and non-zero entries;
    'bwe_dc': predict_bwe with posterior_sampling.data_consistency, the classic replacement step in every evaluation."""
    from babe_amd import degrade as dg
    from babe_amd.testing import model_c, sample_c
    B = 2
    smp, gamma = _edm_sampler(world, dc=task == "bwe_dc")
    _feed_edm(smp, world, gamma, B)
    y0 = world.y[:B].contiguous()
    if task in ("bwe", "bwe_dc"):
        deg, y = dg.FIRDegradation(_fir_taps(33), "cuda"), y0
        want = smp.predict_bwe(y, _fir_taps(33), "firwin")
    elif task in ("inpainting", "compsens"):
        mask = world.mask_row if task == "inpainting" else world.mask_rows
        deg, y = dg.MaskDegradation(mask, "cuda"), (mask * y0).contiguous()
        want = (smp.predict_inpainting if task == "inpainting" else smp.predict_compsens)(y, mask)
    elif task == "declipping":
        deg, y = dg.ClipDegradation(0.05), torch.clip(y0, -0.05, 0.05)
        want = smp.predict_declipping(y, 0.05)
    else:
        deg, y = None, None
        want = smp.predict_unconditional((B, L), "cuda")
    torch.cuda.synchronize()
    dp = smp.diff_params
    rows, t0, _ = sample_c.steps_from(dp, T, smp.order, None, dp.Snoise)
    assert rows[0].inject == 0.0 and rows[1].inject > 0.0
    desc = model_c.observe(world.desc(smp, "per_clip"), deg, dc_classic=task == "bwe_dc")
    got = _lib_run(desc, y, rows, t0, False, _noise_buffer(world, B), skip=True, shape=(B, L))
    assert want.shape == (B, L) and torch.equal(got, want), (task, float((got - want).abs().max()))


def test_seeded_run_equals_the_buffer_run_with_draw_i_plus_1_for_step_i(world):
    """noise = NULL under (seed, clip0) = the buffer run on babe_randn(seed, clip0 + b, k), k = 0 for the initial state and i + 1 for
    step i - on a schedule with a skipped step, which leaves its draw unused and shifts nothing."""
    from babe_amd import degrade as dg
    from babe_amd._lib import check, lib, stream
    from babe_amd.testing import model_c, sample_c
    seed, clip0, B = (1 << 33) + 5, 2, 2
    smp, _ = _edm_sampler(world)
    dp = smp.diff_params
    rows, t0, _ = sample_c.steps_from(dp, T, smp.order, None, dp.Snoise)
    y = world.y[:B].contiguous()
    desc = model_c.observe(world.desc(smp, "per_clip"), dg.FIRDegradation(_fir_taps(33), "cuda"))
    seeded = _lib_run(desc, y, rows, t0, False, None, seed=seed, clip0=clip0, skip=True)
    buf = torch.empty(T + 1, B, L, device="cuda")
    for k in range(T + 1):
        check(lib().babe_randn(buf[k].data_ptr(), L, B, L, seed, clip0, k, stream()), "randn")
    fed = _lib_run(desc, y, rows, t0, False, buf, skip=True)
    assert torch.equal(seeded, fed), float((seeded - fed).abs().max())
    buf[1].zero_()                                     # the skipped step's row is never read
    assert torch.equal(_lib_run(desc, y, rows, t0, False, buf, skip=True), fed)
    other = _lib_run(desc, y, rows, t0, False, None, seed=seed + 1, clip0=clip0, skip=True)
    assert not torch.equal(other, seeded)


@pytest.mark.parametrize("kind", ["iir", "clip"])
def test_workspace_of_the_iir_and_the_clip_kinds_is_exact(world, kind):
    """babe_eval_workspace_bytes is what babe_score_eval takes: one byte less is refused before the first launch."""
    from babe_amd import degrade as dg
    from babe_amd._lib import lib, ptr, stream
    from babe_amd.testing import model_c, sample_c
    smp = _sampler(world, 0)
    deg = dg.make_degradation(_biquad(), "biquad", "cuda")[0] if kind == "iir" else dg.ClipDegradation(0.05)
    d = model_c.observe(world.desc(smp, "per_clip"), deg)
    plain = lib().babe_eval_workspace_bytes(C.byref(world.desc(smp, "per_clip")), 2)
    need = lib().babe_eval_workspace_bytes(C.byref(d), 2)
    assert need > plain > 0                            # the mask bytes (and the IIR workspace) come on top
    y = world.y
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    dd, x_den = torch.empty_like(y), torch.empty_like(y)
    c = sample_c.precond(smp.diff_params, T_EVAL)
    call = lambda nbytes: lib().babe_score_eval(C.byref(d), ptr(y), T_EVAL, *c, ptr(y), None, None, ptr(dd), ptr(x_den), None, ptr(ws),
                                               nbytes, 2, stream())
    dd.fill_(float("nan"))
    assert call(need - 1) < 0 and b"workspace" in lib().babe_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(dd).all()                       # nothing was launched
    assert call(need) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(dd).all() and torch.isfinite(x_den).all()


def test_c_host_with_fir_equals_the_ctypes_run_byte_for_byte(world):
    """examples/c_host/babe_restore --fir 33 2000 300 as a fresh child process on a two-clip input: out.f32 = a ctypes
    babe_sample_bwe call on the same file's model with the FIR of babe_firwin_kaiser in the descriptor, blind = 0, the rows of
    babe_edm_steps under the file's Snoise, the same seed; without the option the host fits the filter and writes other samples; --declip 0.05 equals the ctypes run with the
    clip in the descriptor the same way; a cut-off beyond the Nyquist frequency is refused with the helper's message."""
    from babe_amd import degrade as dg
    from babe_amd._lib import lib
    from babe_amd.build import build_example
    from babe_amd.testing import model_c
    model = world.model()
    tmp = world.tmp
    exe = build_example(out=os.path.join(tmp, "babe_restore"))
    y = world.y
    y.cpu().numpy().tofile(os.path.join(tmp, "in.f32"))

    def run(tag, *extra):
        out = os.path.join(tmp, f"out{tag}.f32")
        r = subprocess.run([exe, world.path, os.path.join(tmp, "in.f32"), out, "--seed", "11", "--batch", "2", *extra],
                           capture_output=True, text=True, timeout=240)
        return r, out

    r, out = run("a", "--fir", "33", "2000", "300")
    assert r.returncode == 0, r.stderr[-3000:]
    x_c = np.fromfile(out, np.float32)
    rows, t0, warm = model_c.edm_steps(model, T, snoise=model.setting("tester.diff_params.Snoise"))
    st = lib().babe_unet_state_create()
    assert st
    try:
        desc = model_c.observe(model.eval_desc(st), dg.FIRDegradation(_fir_taps(33), "cuda"))
        x, _, d = model_c.sample(model, st, y, None, rows, t0, warm, 11, blind=False, desc=desc)
    finally:
        lib().babe_unet_state_destroy(st)
    assert d.eval.obs_kind == 1 and d.eval.ntaps == 33 and x_c.shape == (2 * L,) and np.isfinite(x_c).all()
    assert x_c.tobytes() == x.cpu().numpy().tobytes()
    r, out = run("b")
    assert r.returncode == 0, r.stderr[-3000:]
    assert not np.array_equal(np.fromfile(out, np.float32), x_c)
    # --declip C: the clip in the descriptor, the same way
    r, out = run("d", "--declip", "0.05")
    assert r.returncode == 0, r.stderr[-3000:]
    st = lib().babe_unet_state_create()
    assert st
    try:
        desc = model_c.observe(model.eval_desc(st), dg.ClipDegradation(0.05))
        x, _, d = model_c.sample(model, st, y, None, rows, t0, warm, 11, blind=False, desc=desc)
    finally:
        lib().babe_unet_state_destroy(st)
    assert d.eval.obs_kind == 4 and np.fromfile(out, np.float32).tobytes() == x.cpu().numpy().tobytes()
    r, _ = run("c", "--fir", "32", "20000", "300")
    assert r.returncode == 1 and "--fir" in r.stderr and "cutoff" in r.stderr
