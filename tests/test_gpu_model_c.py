"""csrc/model.hip: a network the library builds from a model file (babe_model_load through testing/model_c.LibraryModel) against
the one the Python engine builds from the same weights - UNet forward and input-VJP, whole sampling runs, the C host of
examples/c_host - bit for bit; and who owns what.  Geometry of tests/test_gpu_sample_c.py.  Needs a MI355X."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS, L, FS, T = [8, 8, 8, 8, 16, 16, 16], 92092, 22050, 3
# The second width.  The nested Winograd kernels need T >= 64, which only levels 0..4 have at this length (level 4: 320 rows x 64
# steps; levels 5 and 6 have 32 and 16 steps, whatever their width).  Ns[4] = 64 puts level 4's six layers on F(4,5) x F(4,3);
# widening levels 5 and 6 changes nothing, so level 3 is widened to 48 channels (no multiple of a 64 / 96 / 128 tile): its five
# layers and the six of the decoder block at level 4 take F(2,5) x F(4,3).
NS_WIDE = [16, 16, 16, 48, 64, 64, 64]


def _args(Ns=NS, **network):
    from babe_amd.config import default_args
    args = default_args(sample_rate=FS, audio_len=L, Ns=Ns, T=T, start_sigma=0.05)
    args.network.update(network)
    return args


def _network(args, sd):
    from babe_amd.networks.cqtdiff_plus import Unet_CQT_oct_with_attention
    net = Unet_CQT_oct_with_attention(args, "cuda")
    net.load_state_dict(sd, strict=True)
    return net


def _export(tmp, name, net, args):
    from babe_amd import model_file
    path = os.path.join(str(tmp), name)
    model_file.export(net, args, path)
    return path


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """One network, its model file, one library-built model of it and one pair of observations for the whole file (never modified)."""
    from babe_amd.networks.cqtdiff_plus import init_state_dict
    from babe_amd.testing.model_c import LibraryModel
    mp = pytest.MonkeyPatch()
    mp.setenv("BABE_CQT_C", "1")                       # the Python sequencer on the library's CQT plan (same tables)
    args = _args()
    net = _network(args, init_state_dict(NS, args.network.num_dils, seed=0, gate_scale=1.0))
    tmp = tmp_path_factory.mktemp("model")
    path = _export(tmp, "small.babe", net, args)
    g = torch.Generator().manual_seed(5)
    y = (0.1 * torch.randn(2, L, generator=g)).cuda()
    model = LibraryModel(path)
    yield dict(net=net, args=args, path=path, model=model, y=y, tmp=tmp)
    model.close()
    mp.undo()


def _unet_case(net, B, seed=3):
    """(C_list, film, gouts) for a UNet evaluation of B rows: CQT coefficients of noise, the engine's FiLM vectors, a cotangent."""
    g = torch.Generator().manual_seed(seed)
    x = (0.1 * torch.randn(B, L, generator=g)).cuda()
    co = [c.contiguous() for c in net.CQTransform.fwd_planar(x)]
    film = net.engine().embed(torch.full((B, 1), 0.3, device="cuda"))
    gouts = [torch.randn(c.shape, generator=g).cuda() for c in co]
    return co, film, gouts


def _unet_equal(net, model, B):
    """babe_unet_fwd + babe_unet_vjp on the model's plan = the same calls on the Python engine's plan, bit for bit."""
    from babe_amd.networks.unet_c import CUnet
    from babe_amd.testing import model_c
    co, film, gouts = _unet_case(net, B)
    py, lb = CUnet(net.engine()), model_c.unet(model)
    want = (py.fwd(co, film), py.vjp(gouts))
    got = (lb.fwd(co, film), lb.vjp(gouts))
    torch.cuda.synchronize()
    for a, b in zip(want[0] + want[1], got[0] + got[1]):
        assert a.shape == b.shape and torch.isfinite(a).all() and a.abs().max() > 0
        assert torch.equal(a, b), float((a - b).abs().max())


@pytest.mark.parametrize("B", [1, 2])
def test_unet_on_the_loaded_plan_equals_the_python_engine(world, B):
    info = world["model"].info
    assert (info.L, info.nocts, info.bpo, list(info.Ns)[:7]) == (L, 7, 64, NS) and info.fs == FS
    assert info.params == sum(v.numel() for v in world["net"].state_dict().values())
    assert info.device == torch.cuda.current_device()
    assert world["model"].setting("tester.T") == T and world["model"].setting("network.Ns.5") == 16
    _unet_equal(world["net"], world["model"], B)


def test_unet_on_a_width_with_both_nested_winograd_kernels(world):
    """NS_WIDE: the library's dispatch counters show F(4,5) x F(4,3) and F(2,5) x F(4,3) launches in the loaded plan's run, so the
    wino85 / wino45 image rules of the loader are exercised in both directions."""
    from babe_amd._lib import dispatch_counts
    from babe_amd.networks.cqtdiff_plus import init_state_dict
    from babe_amd.networks.unet_c import CUnet
    from babe_amd.testing import model_c
    args = _args(NS_WIDE)
    net = _network(args, init_state_dict(NS_WIDE, args.network.num_dils, seed=1, gate_scale=1.0))
    model = model_c.LibraryModel(_export(world["tmp"], "wide.babe", net, args))
    try:
        co, film, gouts = _unet_case(net, 1)
        py = CUnet(net.engine())
        want = py.fwd(co, film) + py.vjp(gouts)
        lb = model_c.unet(model)
        torch.cuda.synchronize()
        dispatch_counts(reset=True)
        got = lb.fwd(co, film) + lb.vjp(gouts)
        torch.cuda.synchronize()
        counts = dispatch_counts()
        assert counts["conv53_wino85"] >= 1 and counts["conv53_wino45"] >= 1, counts
        for a, b in zip(want, got):
            assert torch.isfinite(a).all() and torch.equal(a, b), float((a - b).abs().max())
    finally:
        model.close()


def test_unet_with_folded_frequency_encodings(world):
    """use_fencoding: the loader's 66 -> 2 column convs and babe_fenc_bias tables = the Python engine's."""
    from babe_amd.testing import model_c
    from tests.fencoding_weights import fencoding_sd
    args = _args(use_fencoding=True)
    net = _network(args, fencoding_sd("a"))
    model = model_c.LibraryModel(_export(world["tmp"], "fenc.babe", net, args))
    try:
        _unet_equal(net, model, 2)
    finally:
        model.close()


# ------------------------------------------------------------------------------------------------ sampling runs
def _sampler(world, **kw):
    from babe_amd.diff_params.edm import EDM
    from babe_amd.testing.blind_bwe_sampler import BlindSampler
    args = _args()
    return BlindSampler(world["net"], EDM(args), args, **kw)


def _state():
    from babe_amd._lib import lib
    st = lib().babe_unet_state_create()
    assert st
    return st


def _library_run(world, smp, y, params, blind, seed, rows=None):
    """babe_sample_bwe through LibraryModel.eval_desc with the rows of sample_c.steps_from (or `rows`) -> (x, params, desc)."""
    from babe_amd._lib import lib
    from babe_amd.testing import model_c, sample_c
    if rows is None:
        rows = sample_c.steps_from(smp.diff_params, T, smp.order, smp.start_sigma, 1.0)[:2] + (True,)
    st = _state()
    try:
        return model_c.sample(world["model"], st, y, params, rows[0], rows[1], rows[2], seed, blind=blind)
    finally:
        lib().babe_unet_state_destroy(st)


@pytest.mark.parametrize("B", [1, 2])
def test_blind_run_on_the_loaded_model_equals_the_library_loop(world, B):
    """babe_sample_bwe on LibraryModel.eval_desc = BlindSampler(loop="library", seed=5).predict_blind_bwe(y) in x and the filter
    parameters, per clip; the two descriptors agree in every scalar and in both workspace sizes."""
    from babe_amd._cabi import EvalDesc, SampleDesc
    from babe_amd._lib import lib
    y = world["y"][:B].contiguous()
    smp = _sampler(world, loop="library", seed=5)
    want = smp.predict_blind_bwe(y)
    torch.cuda.synchronize()
    assert smp._csample is not None and smp._csample.calls == 1
    x, p, d = _library_run(world, smp, y, smp._init_params(B, y.device), True, 5)
    assert torch.isfinite(x).all() and torch.equal(x, want[0]), float((x - want[0]).abs().max())
    assert torch.equal(p.reshape(want[1].shape), want[1])
    # the Python-built descriptor of the same run, K and blind set as CSample sets them
    pe = EvalDesc.from_buffer_copy(smp._csample.ce.desc)
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


def test_known_filter_run_on_the_loaded_model(world):
    """predict_bwe(y, filter, 'fc_A') on the library loop = babe_sample_bwe on the loaded model with blind = 0 and that filter."""
    y = world["y"]
    filt = torch.tensor([[3000.0, 5000.0], [-20.0, -40.0]])
    smp = _sampler(world, loop="library", seed=5)
    want = smp.predict_bwe(y, filt, "fc_A")
    torch.cuda.synchronize()
    assert smp._csample is not None and smp._csample.calls == 1
    params = filt.cuda().unsqueeze(0).expand(2, -1, -1).contiguous()
    x, p, _ = _library_run(world, smp, y, params, False, 5)
    assert torch.isfinite(x).all() and torch.equal(x, want) and torch.equal(p, params)


# ------------------------------------------------------------------------------------------------ the C host
def test_c_host_equals_the_ctypes_run_byte_for_byte(world):
    """examples/c_host/babe_restore as a fresh child process: out.f32 and the parameters = a ctypes babe_sample_bwe call on the
    same model file with babe_edm_steps rows, the same seed and batch (both sides on the library's double-precision schedule);
    another seed gives another output."""
    from babe_amd.build import build_example
    from babe_amd.testing import model_c
    tmp = str(world["tmp"])
    exe = build_example(out=os.path.join(tmp, "babe_restore"))
    y = world["y"]
    y.cpu().numpy().tofile(os.path.join(tmp, "in.f32"))

    def run(seed, tag):
        out, par = os.path.join(tmp, f"out{tag}.f32"), os.path.join(tmp, f"par{tag}.f32")
        r = subprocess.run([exe, world["path"], os.path.join(tmp, "in.f32"), out, "--seed", str(seed), "--batch", "2", "--params", par],
                           capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stderr[-3000:]
        return np.fromfile(out, np.float32), np.fromfile(par, np.float32)

    x_c, p_c = run(11, "a")
    smp = _sampler(world)
    rows = model_c.edm_steps(world["model"], T)
    x, p, d = _library_run(world, smp, y, smp._init_params(2, y.device), True, 11, rows=rows)
    assert d.eval.K == 5 and x_c.shape == (2 * L,) and p_c.shape == (2 * 2 * 5,) and np.isfinite(x_c).all()
    assert x_c.tobytes() == x.cpu().numpy().tobytes() and p_c.tobytes() == p.cpu().numpy().tobytes()
    x_o, _ = run(12, "b")
    assert x_o.shape == x_c.shape and not np.array_equal(x_o, x_c)


# ------------------------------------------------------------------------------------------------ ownership
def _hip_runtime():
    """The HIP runtime this process already has loaded (never a second copy)."""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return C.CDLL(line.split()[-1])
    raise RuntimeError("no HIP runtime loaded")


def test_models_own_their_arena(world):
    """Load, destroy, load again; two models alive at once give equal results from separate arenas; device_bytes is the size of
    the allocation the model's pointers live in."""
    from babe_amd.testing import model_c
    first = model_c.LibraryModel(world["path"])
    first.close()
    a, b = model_c.LibraryModel(world["path"]), model_c.LibraryModel(world["path"])
    try:
        co, film, gouts = _unet_case(world["net"], 1)
        res = []
        for m in (a, b, world["model"]):
            cu = model_c.unet(m)
            res.append(cu.fwd(co, film) + cu.vjp(gouts))
        torch.cuda.synchronize()
        for other in res[1:]:
            for u, v in zip(res[0], other):
                assert torch.equal(u, v)
        st = _state()
        da, db = a.eval_desc(st), b.eval_desc(st)
        from babe_amd._lib import lib
        lib().babe_unet_state_destroy(st)
        assert da.rff_freq != db.rff_freq and da.unet_plan != db.unet_plan and da.cqt_plan != db.cqt_plan
        hip = _hip_runtime()
        hip.hipMemGetAddressRange.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_void_p]
        for m, d in ((a, da), (b, db)):
            base, size = C.c_void_p(), C.c_size_t()
            assert hip.hipMemGetAddressRange(C.byref(base), C.byref(size), d.film_W) == 0
            assert size.value == m.info.device_bytes and base.value <= d.rff_freq < base.value + size.value
            assert base.value <= d.env_inv < base.value + size.value and m.info.cqt_device_bytes > 0
    finally:
        a.close()
        b.close()


def test_a_model_is_refused_on_another_device(world):
    if torch.cuda.device_count() < 2:
        pytest.skip("one GPU")
    from babe_amd._lib import BabeHipError
    other = (torch.cuda.current_device() + 1) % torch.cuda.device_count()
    with torch.cuda.device(other):
        for use in (lambda: world["model"].plan, lambda: world["model"].cqt_plan, lambda: world["model"].eval_desc(None)):
            with pytest.raises(BabeHipError, match="lives on device"):
                use()
    assert world["model"].plan


def test_an_attention_network_is_refused_and_nothing_is_left(world):
    """An exported attention fixture: NULL with "attention" in the message, and the device's free memory is what it was."""
    from babe_amd import model_file
    from babe_amd._lib import BabeHipError
    from babe_amd.testing import model_c
    from tests.attention_weights import FIXTURES, fixture_sd
    Ns, fs, La, layers, adict = FIXTURES["a"]
    args = _args(Ns, attention_layers=list(layers), attention_dict=dict(adict))
    path = os.path.join(str(world["tmp"]), "attention.babe")
    model_file.export(fixture_sd("a"), args, path)
    torch.cuda.synchronize()
    free = torch.cuda.mem_get_info()[0]
    with pytest.raises(BabeHipError, match="attention"):
        model_c.LibraryModel(path)
    assert torch.cuda.mem_get_info()[0] == free
