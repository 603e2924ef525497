"""A time-attention network from a model file (babe_model_load_opt with an attention core, testing/model_c.LibraryModel(...,
attention_precision=)) against the Python engine on the same weights: UNet forward and input-VJP, a whole blind sampling run, the
descriptors, who owns the memory, and the C host of examples/c_host with --attention - bit for bit.  Geometry and helpers of
tests/test_gpu_model_c.py; weights of attention fixture `a` (tests/attention_weights.py).  Needs a MI355X."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

from tests.attention_weights import FIXTURES, fixture_sd

pytestmark = pytest.mark.gpu

NS, FS, L, LAYERS, ADICT = FIXTURES["a"]
T = 3


def _args():
    from babe_amd.config import default_args
    args = default_args(sample_rate=FS, audio_len=L, Ns=NS, T=T, start_sigma=0.05)
    args.network.update(attention_layers=list(LAYERS), attention_dict=dict(ADICT))
    return args


class World:
    """The fixture's state_dict, its exported file, and per (precision, attention core) one Python network and one library-built
    model, each made on first use and never modified."""

    def __init__(self, tmp):
        self.tmp, self.args, self.sd = str(tmp), _args(), fixture_sd("a")
        self.path = os.path.join(self.tmp, "attention.babe")
        from babe_amd import model_file
        model_file.export(self.sd, self.args, self.path)
        g = torch.Generator().manual_seed(5)
        self.y = (0.1 * torch.randn(2, L, generator=g)).cuda()
        self._nets, self._models = {}, {}

    def net(self, precision="f32", core="f32"):
        from babe_amd.networks.cqtdiff_plus import Unet_CQT_oct_with_attention
        if (precision, core) not in self._nets:
            net = Unet_CQT_oct_with_attention(self.args, "cuda", precision=precision, attention_precision=core)
            net.load_state_dict(self.sd, strict=True)
            self._nets[precision, core] = net
        return self._nets[precision, core]

    def model(self, precision="f32", core="f32"):
        from babe_amd.testing.model_c import LibraryModel
        if (precision, core) not in self._models:
            self._models[precision, core] = LibraryModel(self.path, precision, attention_precision=core)
        return self._models[precision, core]

    def close(self):
        for m in self._models.values():
            m.close()


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    mp = pytest.MonkeyPatch()
    mp.setenv("BABE_CQT_C", "1")                       # the Python sequencer on the library's CQT plan (same tables)
    w = World(tmp_path_factory.mktemp("attention_model"))
    yield w
    w.close()
    mp.undo()


def _unet_case(net, B, seed=3):
    g = torch.Generator().manual_seed(seed)
    x = (0.1 * torch.randn(B, L, generator=g)).cuda()
    co = [c.contiguous() for c in net.CQTransform.fwd_planar(x)]
    film = net.engine().embed(torch.full((B, 1), 0.3, device="cuda"))
    gouts = [torch.randn(c.shape, generator=g).cuda() for c in co]
    return co, film, gouts


def _unet_equal(net, model, B):
    """babe_unet_fwd + babe_unet_vjp on the model's plan = the same calls on the Python engine's attention plan, bit for bit."""
    from babe_amd.networks.unet_c import CUnet
    from babe_amd.testing import model_c
    co, film, gouts = _unet_case(net, B)
    py, lb = CUnet(net.engine(), attention=True), model_c.unet(model)
    want = py.fwd(co, film) + py.vjp(gouts)
    got = lb.fwd(co, film) + lb.vjp(gouts)
    torch.cuda.synchronize()
    for a, b in zip(want, got):
        assert a.shape == b.shape and torch.isfinite(a).all() and a.abs().max() > 0
        assert torch.equal(a, b), float((a - b).abs().max())


@pytest.mark.parametrize("B", [1, 2])
def test_unet_on_the_loaded_attention_plan_equals_the_python_engine(world, B):
    model = world.model()
    info = model.info
    assert model.attention == 1 and model.precision == 0
    assert (info.L, info.nocts, info.bpo, list(info.Ns)[:7]) == (L, 7, 64, NS) and info.fs == FS
    assert info.params == sum(v.numel() for v in world.sd.values())
    assert model.setting("network.attention_layers.4") == 1 and model.setting("network.attention_dict.num_heads") == 8
    _unet_equal(world.net(), model, B)


@pytest.mark.parametrize("B", [1, 2])
def test_bf16_network_on_the_bf16_core(world, B):
    """precision = bf16 with the bf16 attention core, against the Python network built the same way from the same fp32 weights."""
    model = world.model("bf16", "bf16")
    assert model.attention == 2 and model.precision == 1
    net = world.net("bf16", "bf16")
    assert net.engine().precision == "bf16" and net.engine().attn_core == "bf16"
    _unet_equal(net, model, B)


# ------------------------------------------------------------------------------------------------ a sampling run
def _sampler(world, **kw):
    from babe_amd.diff_params.edm import EDM
    from babe_amd.testing.blind_bwe_sampler import BlindSampler
    return BlindSampler(world.net(), EDM(world.args), world.args, **kw)


def _state():
    from babe_amd._lib import lib
    st = lib().babe_unet_state_create()
    assert st
    return st


def _library_run(world, smp, y, seed, rows=None):
    from babe_amd._lib import lib
    from babe_amd.testing import model_c, sample_c
    if rows is None:
        rows = sample_c.steps_from(smp.diff_params, T, smp.order, smp.start_sigma, 1.0)[:2] + (True,)
    st = _state()
    try:
        return model_c.sample(world.model(), st, y, smp._init_params(y.shape[0], y.device), rows[0], rows[1], rows[2], seed, blind=True)
    finally:
        lib().babe_unet_state_destroy(st)


@pytest.mark.parametrize("B", [1, 2])
def test_blind_run_on_the_loaded_model_equals_the_python_loop(world, B, monkeypatch):
    """babe_sample_bwe on LibraryModel.eval_desc = BlindSampler(loop="python", noise_device="philox", seed).predict_blind_bwe(y) in x
    and the filter parameters (the identity tests/test_gpu_sample_c.py shows without attention); the Python-built descriptor
    over the engine's attention plan and the library-built one agree in every scalar and in both workspace sizes."""
    from babe_amd._cabi import EvalDesc, SampleDesc
    from babe_amd._lib import lib
    from babe_amd.networks import unet_c
    from babe_amd.testing import eval_c
    seed = 5
    y = world.y[:B].contiguous()
    smp = _sampler(world, loop="python", noise_device="philox", seed=seed)
    want = smp.predict_blind_bwe(y)
    torch.cuda.synchronize()
    assert smp._csample is None                                   # the Python loop, on the Python sequencer
    x, p, d = _library_run(world, smp, y, seed)
    assert torch.isfinite(x).all() and x.abs().max() > 0
    assert torch.equal(x, want[0]), float((x - want[0]).abs().max())
    assert torch.equal(p.reshape(want[1].shape), want[1])
    # the Python-built descriptor of the same run: CEval over the engine's plan, asked for with the attention opt-in
    monkeypatch.setattr(unet_c, "CUnet", functools.partial(unet_c.CUnet, attention=True))
    smp.stft_ops(L, y.device)
    ce = eval_c.CEval(smp, 0)
    pe = EvalDesc.from_buffer_copy(ce.desc)
    pe.K, pe.blind = d.eval.K, d.eval.blind
    for f in ("L", "rff_n", "film_J", "nfft", "fs", "K", "blind", "shared", "hpf", "xi", "score_mode", "audio_len_norm"):
        assert getattr(pe, f) == getattr(d.eval, f), f
    assert list(pe.emb_dim) == list(d.eval.emb_dim) and bytes(pe.fit) == bytes(d.eval.fit)
    pd = SampleDesc.from_buffer_copy(d)
    pd.eval = pe
    for b in (1, 2):
        n = lib().babe_eval_workspace_bytes(C.byref(pe), b)
        assert n > 0 and n == lib().babe_eval_workspace_bytes(C.byref(d.eval), b)
        n = lib().babe_sample_workspace_bytes(C.byref(pd), b)
        assert n > 0 and n == lib().babe_sample_workspace_bytes(C.byref(d), b)


# ------------------------------------------------------------------------------------------------ ownership, the C host
def test_close_and_reload_leave_free_memory_unchanged(world):
    from babe_amd.testing.model_c import LibraryModel
    LibraryModel(world.path, attention_precision="f32").close()
    torch.cuda.synchronize()
    free = torch.cuda.mem_get_info()[0]
    m = LibraryModel(world.path, attention_precision="f32")
    assert torch.cuda.mem_get_info()[0] <= free - m.info.device_bytes
    m.close()
    assert torch.cuda.mem_get_info()[0] == free


def test_c_host_with_attention_equals_the_ctypes_run_byte_for_byte(world):
    """examples/c_host/babe_restore --attention f32 as a fresh child process: out.f32 and the parameters = a ctypes babe_sample_bwe
    call on the same file with babe_edm_steps rows, the same seed and batch; without the flag the host refuses the file."""
    from babe_amd.build import build_example
    from babe_amd.testing import model_c
    exe = build_example(out=os.path.join(world.tmp, "babe_restore"))
    y = world.y
    src = os.path.join(world.tmp, "in.f32")
    y.cpu().numpy().tofile(src)
    out, par = os.path.join(world.tmp, "out.f32"), os.path.join(world.tmp, "par.f32")
    cmd = [exe, world.path, src, out, "--seed", "11", "--batch", "2", "--params", par]
    r = subprocess.run(cmd + ["--attention", "f32"], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    x_c, p_c = np.fromfile(out, np.float32), np.fromfile(par, np.float32)
    smp = _sampler(world)
    x, p, d = _library_run(world, smp, y, 11, rows=model_c.edm_steps(world.model(), T))
    assert d.eval.K == 5 and x_c.shape == (2 * L,) and p_c.shape == (2 * 2 * 5,) and np.isfinite(x_c).all()
    assert x_c.tobytes() == x.cpu().numpy().tobytes() and p_c.tobytes() == p.cpu().numpy().tobytes()
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    assert r.returncode != 0 and "attention" in r.stderr, (r.returncode, r.stderr[-1000:])
    r = subprocess.run(cmd + ["--attention", "fp16"], capture_output=True, text=True, timeout=240)
    assert r.returncode == 1 and "--attention" in r.stderr
