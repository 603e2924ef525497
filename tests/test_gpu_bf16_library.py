"""bf16 / bf16x3 networks on the library path: the C sequencer (csrc/unet_engine.hip) against the Python sequencer over ONE engine's
images - the units branch included -, a network babe_model_load_ex packs from the fp32 file against the Python bf16 engine, and whole
runs (babe_sample_bwe, babe_restore_recording, the C host) on the loaded bf16 model against the Python bf16 loop.  Both sides
launch the same kernels on the same images in the same order: every comparison is torch.equal.  Geometry of
tests/test_gpu_model_c.py.  Needs a MI355X."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NS, L, FS, T = [8, 8, 8, 8, 16, 16, 16], 92092, 22050, 3
# levels 3..6 (48 / 64 channels; 128, 64, 32, 16 time steps, all multiples of 4) take bf16 units; levels 0..2 run the bf16 kernels
# over fp32 activations; the 2-channel and the narrow (1,1) convs stay on the fp32 kernels
NS_WIDE = [16, 16, 16, 48, 64, 64, 64]
WIDTHS = {"small": NS, "wide": NS_WIDE}
OVERLAP = 5512


def _args(Ns=NS, **network):
    from babe_amd.config import default_args
    args = default_args(sample_rate=FS, audio_len=L, Ns=Ns, T=T, start_sigma=0.05)
    args.network.update(network)
    return args


def _network(args, sd, precision):
    from babe_amd.networks.cqtdiff_plus import Unet_CQT_oct_with_attention
    net = Unet_CQT_oct_with_attention(args, "cuda", precision=precision)
    net.load_state_dict(sd, strict=True)
    return net


class _World:
    """State dicts, Python networks per (width, precision), exported fp32 files and library-built models per (width, precision),
    each made once on first use and never modified."""

    def __init__(self, tmp):
        self.tmp, self._sd, self._nets, self._paths, self._models = str(tmp), {}, {}, {}, {}
        g = torch.Generator().manual_seed(5)
        self.y = (0.1 * torch.randn(2, L, generator=g)).cuda()

    def args(self, width):
        return _args(WIDTHS[width])

    def sd(self, width):
        from babe_amd.networks.cqtdiff_plus import init_state_dict
        if width not in self._sd:
            a = self.args(width)
            self._sd[width] = init_state_dict(WIDTHS[width], a.network.num_dils, seed=len(width), gate_scale=1.0)
        return self._sd[width]

    def net(self, width, precision):
        if (width, precision) not in self._nets:
            self._nets[width, precision] = _network(self.args(width), self.sd(width), precision)
        return self._nets[width, precision]

    def path(self, width):
        from babe_amd import model_file
        if width not in self._paths:
            self._paths[width] = os.path.join(self.tmp, width + ".babe")
            model_file.export(self.sd(width), self.args(width), self._paths[width])
        return self._paths[width]

    def model(self, width, precision):
        from babe_amd.testing.model_c import LibraryModel
        if (width, precision) not in self._models:
            self._models[width, precision] = LibraryModel(self.path(width), precision)
        return self._models[width, precision]

    def close(self):
        for m in self._models.values():
            m.close()


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    mp = pytest.MonkeyPatch()
    mp.setenv("BABE_CQT_C", "1")                       # the Python sequencer on the library's CQT plan (same tables)
    w = _World(tmp_path_factory.mktemp("bf16"))
    yield w
    w.close()
    mp.undo()


def _unet_case(net, B, seed=3):
    """(C_list, film, gouts) for a UNet evaluation of B rows: CQT coefficients of noise, the engine's FiLM vectors, a cotangent."""
    g = torch.Generator().manual_seed(seed)
    x = (0.1 * torch.randn(B, L, generator=g)).cuda()
    co = [c.contiguous() for c in net.CQTransform.fwd_planar(x)]
    film = net.engine().embed(torch.full((B, 1), 0.3, device="cuda"))
    gouts = [torch.randn(c.shape, generator=g).cuda() for c in co]
    return co, film, gouts


def _all_equal(want, got):
    assert len(want) == len(got)
    for a, b in zip(want, got):
        assert a.shape == b.shape and torch.isfinite(a).all() and a.abs().max() > 0
        assert torch.equal(a, b), float((a - b).abs().max())


def _counted(run):
    from babe_amd._lib import dispatch_counts
    torch.cuda.synchronize()
    dispatch_counts(reset=True)
    res = run()
    torch.cuda.synchronize()
    return res, dispatch_counts(reset=True)


# ------------------------------------------------------------------------------------------------ two sequencers, one engine
@pytest.mark.parametrize("precision,width,B", [("bf16", "small", 1), ("bf16", "small", 2), ("bf16", "wide", 1), ("bf16", "wide", 2),
                                               ("bf16x3", "wide", 1)])
def test_c_sequencer_equals_the_python_sequencer_on_one_engine(world, precision, width, B):
    """CUnet(engine) - babe_unet_fwd / babe_unet_vjp, in exactly babe_unet_workspace_bytes bytes - against the same engine's
    Python-sequenced forward / vjp: equal outputs and gradients, and the same number of launches in every slot of the library's
    dispatch counters.  One slot differs by construction when B > 1: the C sequencer makes each layer's gate rows contiguous with
    babe_axpby4d (slot "axpby") where the Python sequencer uses torch's copy, one launch per dilation layer.
    babe_scale_gelu_units reports to the slot "scale_gelu" (as babe_scale_gelu_fin does), babe_conv2d_bf16_units to "conv_bf16p";
    the units layers themselves are counted through "gn_stats" (below): on the wide network under bf16 every layer the static
    rule names took units - levels 3..6, 52 of the 90 layers, measured on a MI355X - and none anywhere else."""
    from babe_amd._lib import lib
    from babe_amd.networks.unet_c import CUnet
    net = world.net(width, precision)
    eng = net.engine()
    assert eng.precision == precision and eng._c_engine() is None        # the Python sequencer stays the engine's own path
    co, film, gouts = _unet_case(net, B)
    want, n_py = _counted(lambda: eng.forward(co, film) + eng.vjp(gouts))
    cu = CUnet(eng)
    got, n_c = _counted(lambda: cu.fwd(co, film) + cu.vjp(gouts))
    _all_equal(want, got)
    n = len(co)
    T_oct = (C.c_int * n)(*[int(c.shape[-1]) for c in co])
    assert cu.ws.numel() == lib().babe_unet_workspace_bytes(cu.plan, B, T_oct)
    layers = sum(b.nd for b in eng.blocks())
    expect = dict(n_py)
    if B > 1:
        expect["axpby"] += layers
    print(f"{precision} {width} B={B}: python {n_py}\n  library {n_c}")
    assert n_c == expect, {k: (n_c[k], expect[k]) for k in n_c if n_c[k] != expect[k]}
    # Which layers took units: a units layer launches babe_gn_partial AND babe_gn_finalize (two launches in "gn_stats"), any other
    # layer babe_gn_partial alone (the finalize is inside its GELU launch; no conv forms GroupNorm sums over bf16 images).  The
    # expected number is the static rule asked block by block at that block's time length.
    Ts = [int(co[n - 1 - i].shape[-1]) for i in range(n)]          # level i
    at = [(eng.init_blk[i], Ts[i]) for i in range(n)] + [(eng.main_blk[i], Ts[i]) for i in range(n)] + \
        [(eng.mid_blk, Ts[n - 1]), (eng.mid_out, Ts[n - 1])] + \
        [(eng.up_out[i], Ts[n - 1 - i]) for i in range(n)] + [(eng.up_blk[i], Ts[n - 1 - i]) for i in range(n)]
    assert sum(b.nd for b, _ in at) == layers
    units = sum(b.nd for b, t in at if b.nd and lib().babe_conv2d_bf16_units_shape(C.byref(b.H[0].desc), t))
    assert n_c["gn_stats"] == layers + units and n_c["scale_gelu"] == layers      # one GELU launch per layer: units or fp32
    if width == "wide" and precision == "bf16":
        assert 0 < units < layers and n_c["conv_bf16p"] >= units
    else:
        assert units == 0
    if precision == "bf16x3":
        assert n_c["conv_bf16"] > 0                        # the three-product kernels, over fp32 activations


# ------------------------------------------------------------------------------------------------ the loaded model
def _loaded_equals_python(world, net, model, B):
    from babe_amd.networks.unet_c import CUnet
    from babe_amd.testing import model_c
    co, film, gouts = _unet_case(net, B)
    py, lb = CUnet(net.engine()), model_c.unet(model)
    want = py.fwd(co, film) + py.vjp(gouts)
    got = lb.fwd(co, film) + lb.vjp(gouts)
    torch.cuda.synchronize()
    _all_equal(want, got)


@pytest.mark.parametrize("width,B", [("small", 2), ("wide", 1)])
def test_loaded_bf16_model_equals_the_python_bf16_engine(world, width, B):
    """LibraryModel(fp32 file, "bf16"): its plan runs to the same bits as the plan over the Python bf16 engine of the same state
    dict; babe_model_precision says 1; the arena is smaller than the fp32 model's (bf16 images, no Winograd images)."""
    model = world.model(width, "bf16")
    assert model.precision == 1 and world.model(width, "f32").precision == 0
    assert model.info.device_bytes < world.model(width, "f32").info.device_bytes
    assert model.info.params == sum(v.numel() for v in world.sd(width).values())
    _loaded_equals_python(world, world.net(width, "bf16"), model, B)


def test_loaded_bf16x3_model_equals_the_python_engine(world):
    model = world.model("wide", "bf16x3")
    assert model.precision == 2
    _loaded_equals_python(world, world.net("wide", "bf16x3"), model, 1)


def test_loaded_images_are_packed_convs_buffers(world):
    """Per conv of the Python bf16 engine: babe_packed_conv_plan for (shape, babe_conv_splits_for(shape, 1, 1)) with the loader's
    arguments gives the byte count of every buffer the PackedConv holds."""
    from babe_amd._cabi import IMAGE_SLOTS, PackedConvLayout
    from babe_amd._lib import lib
    eng = world.net("wide", "bf16").engine()
    kinds = set()
    for _, pc in eng.packs:
        shape = (pc.Cout, pc.Cin, pc.KH, pc.KW)
        splits = lib().babe_conv_splits_for(*shape, 1, 1)
        assert splits == pc.splits
        kinds.add(splits)
        lay = PackedConvLayout()
        assert lib().babe_packed_conv_plan(*shape, splits, 0, 2, 31, C.byref(lay)) == 0
        for name, nbytes in zip(IMAGE_SLOTS, lay.bytes):
            t = getattr(pc, name)
            assert (t.numel() * t.element_size() if t is not None else 0) == nbytes, (shape, name)
    assert kinds == {0, 1}


def test_use_fencoding_file_loads_as_bf16(world):
    """The folded 66 -> 2 column convs stay fp32 images under any precision, so a use_fencoding file loads as bf16 and runs to
    the Python bf16 engine's bits."""
    from babe_amd import model_file
    from babe_amd.testing import model_c
    from tests.fencoding_weights import fencoding_sd
    args = _args(use_fencoding=True)
    sd = fencoding_sd("a")
    path = os.path.join(world.tmp, "fenc.babe")
    model_file.export(sd, args, path)
    model = model_c.LibraryModel(path, "bf16")
    try:
        assert model.precision == 1
        _loaded_equals_python(world, _network(args, sd, "bf16"), model, 2)
    finally:
        model.close()


def test_fp32_load_is_what_it_was(world):
    """LibraryModel(path) and LibraryModel(path, "f32"): the same arena size and the same UNet workspace size - and an fp32 plan
    carves no units buffer: its workspace is the Python fp32 engine's plan's."""
    from babe_amd._lib import lib
    from babe_amd.testing.model_c import LibraryModel
    for width in ("small", "wide"):
        a, b = LibraryModel(world.path(width)), world.model(width, "f32")
        try:
            assert a.precision == 0 and a.info.device_bytes == b.info.device_bytes
            co, _, _ = _unet_case(world.net(width, "bf16"), 1)
            T_oct = (C.c_int * len(co))(*[int(c.shape[-1]) for c in co])
            for B in (1, 2):
                n = lib().babe_unet_workspace_bytes(a.plan, B, T_oct)
                assert n > 0 and n == lib().babe_unet_workspace_bytes(b.plan, B, T_oct)
                nb = lib().babe_unet_workspace_bytes(world.model(width, "bf16").plan, B, T_oct)
                assert (nb > n) if width == "wide" else (nb == n)          # the units buffer, only where a block takes units
        finally:
            a.close()


# ------------------------------------------------------------------------------------------------ sampling runs
def _sampler(world, **kw):
    from babe_amd.diff_params.edm import EDM
    from babe_amd.testing.blind_bwe_sampler import BlindSampler
    args = world.args("small")
    return BlindSampler(world.net("small", "bf16"), EDM(args), args, **kw)


def _state():
    from babe_amd._lib import lib
    st = lib().babe_unet_state_create()
    assert st
    return st


@pytest.mark.parametrize("blind,B", [(True, 1), (True, 2), (False, 1), (False, 2)])
def test_sampling_run_on_the_bf16_model_equals_the_python_bf16_loop(world, blind, B):
    """babe_sample_bwe on LibraryModel(path, "bf16").eval_desc with the rows of sample_c.steps_from = BlindSampler(bf16 network,
    loop="python", seed=s, noise_device="philox") in x and the filter parameters; the Python sampler has no library run to fall
    back from (sample_c.supported is False for a bf16 network)."""
    from babe_amd._lib import lib
    from babe_amd.testing import model_c, sample_c
    seed = 5
    y = world.y[:B].contiguous()
    smp = _sampler(world, loop="python", seed=seed, noise_device="philox")
    assert not sample_c.supported(smp, y, blind, False)
    filt = torch.tensor([[3000.0, 5000.0], [-20.0, -40.0]])
    if blind:
        want_x, want_p = smp.predict_blind_bwe(y)
        params = smp._init_params(B, y.device)
    else:
        want_x = smp.predict_bwe(y, filt, "fc_A")
        params = want_p = filt.cuda().unsqueeze(0).expand(B, -1, -1).contiguous()
    torch.cuda.synchronize()
    assert smp._csample is None
    rows, t0, _ = sample_c.steps_from(smp.diff_params, T, smp.order, smp.start_sigma, 1.0 if blind else smp.diff_params.Snoise)
    st = _state()
    try:
        x, p, _ = model_c.sample(world.model("small", "bf16"), st, y, params, rows, t0, True, seed, blind=blind)
    finally:
        lib().babe_unet_state_destroy(st)
    assert torch.isfinite(x).all() and float(x.abs().max()) > 0
    assert torch.equal(x, want_x), float((x - want_x).abs().max())
    assert torch.equal(p.reshape(want_p.shape), want_p)


def test_bf16_run_differs_from_the_fp32_run(world):
    """The precision reaches the run: the same call on the fp32 model of the same file gives other samples."""
    from babe_amd._lib import lib
    from babe_amd.testing import model_c, sample_c
    y = world.y[:1].contiguous()
    smp = _sampler(world)
    rows, t0, _ = sample_c.steps_from(smp.diff_params, T, smp.order, smp.start_sigma, 1.0)
    xs = []
    for precision in ("f32", "bf16"):
        st = _state()
        try:
            xs.append(model_c.sample(world.model("small", precision), st, y, smp._init_params(1, y.device), rows, t0, True, 5)[0])
        finally:
            lib().babe_unet_state_destroy(st)
    assert not torch.equal(xs[0], xs[1]) and float((xs[0] - xs[1]).abs().max()) < 0.1


# ------------------------------------------------------------------------------------------------ a recording
def test_recording_on_the_bf16_model_equals_the_python_bf16_flow(world):
    """babe_restore_recording on the bf16 model's descriptor = restore_recording_complete on the Python bf16 sampler (Python loop,
    the library's generator) with the same seed, clip0 and blind segment: one blind segment, then a walk of two segments (the
    second out-painted from the first and cut short by the file's end).  The restored file, the filter and the blind step's
    restoration are equal."""
    from babe_amd._cabi import RecordingDesc
    from babe_amd._lib import check, lib, ptr, stream
    from babe_amd.testing import sample_c
    from babe_amd.testing.long_file import restore_recording_complete
    from tests.test_gpu_recording_c import _Starts, synth_recording
    seed, lrec, starts, size = 3, 150000, [0], 50
    rec = synth_recording(lrec, FS, 2).cuda()
    seg_starts, seg_valid = (C.c_long * 3)(), (C.c_long * 3)()
    assert lib().babe_recording_plan(lrec, L, OVERLAP, 200, seg_starts, seg_valid, 3) == 2 and seg_valid[1] < L
    smp = _sampler(world, loop="python", seed=seed, noise_device="philox")
    want = restore_recording_complete(smp, rec, n_segments_blindstep=len(starts), rng=_Starts(starts), clip0=0)
    torch.cuda.synchronize()
    assert smp._csample is None
    want = tuple(r.clone() for r in want)

    model = world.model("small", "bf16")
    st = _state()
    try:
        args, dp = smp.args, smp.diff_params
        d = RecordingDesc()
        d.eval = model.eval_desc(st)
        init = smp._init_params(1, rec.device)[0].contiguous()
        rows_b, t0, _ = sample_c.steps_from(dp, T, smp.order, smp.start_sigma, 1.0)
        rows_k, _, _ = sample_c.steps_from(dp, T, smp.order, smp.start_sigma, dp.Snoise)
        window = torch.hann_window(2 * size).to(rec.device)
        d.eval.K, d.eval.shared = int(init.shape[-1]), 0
        d.T, d.t0, d.warm_start, d.steps_blind, d.steps_known = T, t0, 1, rows_b, rows_k
        d.n_blind = len(starts)
        d.blind_starts[0] = starts[0]
        d.init_params, d.target_std = ptr(init), 0.1
        d.overlap, d.discard_end = int(0.25 * FS), 200
        d.inpaint_dc, d.dc_size, d.dc_window = int(bool(args.tester.complete_recording.inpaint_DC)), size, ptr(window)
        s = rec.reshape(1, -1).std(-1)                     # torch's standard deviation of the file, as the Python flow takes it
        d.std_dev = ptr(s)
        assert d.overlap == OVERLAP
        out, filt, pred = torch.empty(lrec, device="cuda"), torch.empty(2, d.eval.K, device="cuda"), torch.empty(1, L, device="cuda")
        need = lib().babe_recording_workspace_bytes(C.byref(d))
        assert need > 0, lib().babe_last_error()
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        check(lib().babe_restore_recording(C.byref(d), ptr(rec), lrec, ptr(out), ptr(filt), ptr(pred), seed, 0, ptr(ws), need, stream()),
              "restore_recording")
        torch.cuda.synchronize()
    finally:
        lib().babe_unet_state_destroy(st)
    assert torch.isfinite(out).all() and float(out.abs().max()) > 0
    assert torch.equal(filt, want[1].reshape(filt.shape)), (filt, want[1])
    assert torch.equal(pred, want[2]), float((pred - want[2]).abs().max())
    assert torch.equal(out, want[0]), float((out - want[0]).abs().max())


# ------------------------------------------------------------------------------------------------ the C host
def test_c_host_with_precision_bf16_equals_the_ctypes_run_byte_for_byte(world):
    """examples/c_host/babe_restore --precision bf16 as a fresh child process: out.f32 and the parameters = a ctypes babe_sample_bwe
    call on LibraryModel(path, "bf16") with babe_edm_steps rows, the same seed and batch; without the option the host runs the
    fp32 network and writes other samples; a precision it does not know is refused."""
    from babe_amd._lib import lib
    from babe_amd.build import build_example
    from babe_amd.testing import model_c
    tmp = world.tmp
    exe = build_example(out=os.path.join(tmp, "babe_restore"))
    y = world.y
    y.cpu().numpy().tofile(os.path.join(tmp, "in.f32"))

    def run(tag, *extra):
        out, par = os.path.join(tmp, f"out{tag}.f32"), os.path.join(tmp, f"par{tag}.f32")
        r = subprocess.run([exe, world.path("small"), os.path.join(tmp, "in.f32"), out, "--seed", "11", "--batch", "2", "--params", par,
                            *extra], capture_output=True, text=True, timeout=240)
        return r, out, par

    r, out, par = run("a", "--precision", "bf16")
    assert r.returncode == 0, r.stderr[-3000:]
    x_c, p_c = np.fromfile(out, np.float32), np.fromfile(par, np.float32)
    model = world.model("small", "bf16")
    rows = model_c.edm_steps(model, T)
    st = _state()
    try:
        x, p, d = model_c.sample(model, st, y, _sampler(world)._init_params(2, y.device), rows[0], rows[1], rows[2], 11, blind=True)
    finally:
        lib().babe_unet_state_destroy(st)
    assert d.eval.K == 5 and x_c.shape == (2 * L,) and p_c.shape == (2 * 2 * 5,) and np.isfinite(x_c).all()
    assert x_c.tobytes() == x.cpu().numpy().tobytes() and p_c.tobytes() == p.cpu().numpy().tobytes()
    r, out, _ = run("b")
    assert r.returncode == 0, r.stderr[-3000:]
    x_f = np.fromfile(out, np.float32)
    assert x_f.shape == x_c.shape and not np.array_equal(x_f, x_c)
    r, _, _ = run("c", "--precision", "fp16")
    assert r.returncode == 1 and "--precision" in r.stderr
