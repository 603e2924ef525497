"""csrc/recording.hip: a whole recording restored by ONE C-ABI call (babe_restore_recording; long_file.restore_recording_library)
against the Python flow long_file.restore_recording_complete sequencing the same kernels under the same noise numbering, bit for
bit; the driver's own kernels one by one; the C host examples/c_host/babe_restore_recording as a child process.  Network and
segment length of tests/test_gpu_sample_c.py.  Needs a MI355X."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NS, L, FS, T = [8, 8, 8, 8, 16, 16, 16], 92092, 22050, 3
LREC, STARTS, SEED = 240000, [0, 40000], 3            # one first segment, one AR segment, one short last segment
OVERLAP, SIZE = 5512, 50


def _args():
    from babe_amd.config import default_args
    return default_args(sample_rate=FS, audio_len=L, Ns=NS, T=T, start_sigma=0.05)


def synth_recording(n, fs, seed):
    """The synthetic recording of tests/test_gpu_flows.py::synth_recording, restated: decaying harmonics plus noise, low-passed."""
    from oracle import bwe_utils as U
    g = torch.Generator().manual_seed(seed)
    t_ax = torch.arange(n) / fs
    clean = sum(0.05 / (k + 1) * torch.sin(2 * np.pi * 196.0 * (k + 1) * t_ax) * torch.exp(-(t_ax % 2.0) * (1 + k)) for k in range(12))
    clean = clean + 0.1 * torch.randn(n, generator=g)
    f = torch.fft.rfftfreq(4096, d=1 / fs)
    return U.apply_filter(clean[None], U.design_filter(torch.tensor([2500.0]), torch.tensor([-35.0]), f), 4096)[0]


class _Starts:
    """Stands in for numpy's generator: restore_recording_complete draws the blind segments' starts from it."""

    def __init__(self, starts):
        self.it = iter(starts)

    def randint(self, lo, hi):
        v = next(self.it)
        assert lo <= v < hi
        return v


@pytest.fixture(scope="module")
def world():
    from babe_amd.networks.cqtdiff_plus import Unet_CQT_oct_with_attention, init_state_dict
    mp = pytest.MonkeyPatch()
    mp.setenv("BABE_CQT_C", "1")                       # the Python sequencer on the library's CQT plan (same tables)
    args = _args()
    net = Unet_CQT_oct_with_attention(args, "cuda")
    net.load_state_dict(init_state_dict(NS, args.network.num_dils, seed=0, gate_scale=1.0))
    yield dict(net=net, args=args, rec=synth_recording(LREC, FS, 2).cuda())
    mp.undo()


def _sampler(world, **kw):
    from babe_amd.diff_params.edm import EDM
    from babe_amd.testing.blind_bwe_sampler import BlindSampler
    args = _args()
    return BlindSampler(world["net"], EDM(args), args, **kw)


def _python_flow(world, rec, starts):
    """restore_recording_complete(..., clip0=0) on a fresh sampler: the Python loop on the library's generator."""
    from babe_amd.testing.long_file import restore_recording_complete
    smp = _sampler(world, loop="python", seed=SEED, noise_device="philox")
    res = restore_recording_complete(smp, rec, n_segments_blindstep=len(starts), rng=_Starts(starts), clip0=0)
    torch.cuda.synchronize()
    assert smp._csample is None
    return tuple(r.clone() for r in res)


def _library_flow(world, rec, starts, std_dev):
    from babe_amd.testing.long_file import restore_recording_library
    res = restore_recording_library(_sampler(world, loop="library", seed=SEED), rec, blind_starts=starts, clip0=0, std_dev=std_dev)
    torch.cuda.synchronize()
    return tuple(r.clone() for r in res)


@pytest.fixture(scope="module")
def flows(world):
    """The 240000-sample recording through the Python flow and through the one-call driver (handed torch's standard deviation, and
    measuring its own), once for the tests below."""
    rec = world["rec"]
    s = rec.reshape(1, -1).std(-1)
    return dict(py=_python_flow(world, rec, STARTS), lib=_library_flow(world, rec, STARTS, s), own=_library_flow(world, rec, STARTS, None))


# ------------------------------------------------------------------------------------------------ the driver's kernels
def _ulps(a, b):
    ia = np.asarray(a, np.float32).view(np.int32).astype(np.int64)
    ib = np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    return np.abs(ia - ib)


def test_row_std_against_float64():
    """babe_row_std against numpy's float64 std(ddof=1) rounded to float32: at most 2 ulp (double accumulation adds less than
    n 2^-53 relative; the square root and the final rounding one ulp each); rows that start off a 16-byte boundary and rows with
    an offset much larger than their spread included; two calls give the same bits; one sample is refused."""
    from babe_amd._lib import lib, stream
    g = torch.Generator().manual_seed(7)
    part = torch.empty(2 * 128, dtype=torch.float64, device="cuda")
    for n in (2, 255, 256, 257, 92092):
        for off in (0, 1, 3):
            for dc in (0.0, 30.0):
                base = (0.1 * torch.randn(2 * (n + 4), generator=g) + dc).cuda()
                x_bs = n + 4
                out = torch.empty(2, device="cuda")
                call = lambda o: lib().babe_row_std(base.data_ptr() + 4 * off, x_bs, 2, n, o.data_ptr(), part.data_ptr(), stream())
                assert call(out) == 0
                again = torch.empty(2, device="cuda")
                assert call(again) == 0
                rows = base.cpu().numpy()[off:].astype(np.float64)
                want = np.stack([rows[b * x_bs:b * x_bs + n].std(ddof=1) for b in range(2)]).astype(np.float32)
                got = out.cpu().numpy()
                assert np.isfinite(got).all() and _ulps(got, want).max() <= 2, (n, off, dc, got, want)
                assert torch.equal(out, again)
    x = torch.ones(4, device="cuda")
    assert lib().babe_row_std(x.data_ptr(), 4, 1, 1, x.data_ptr(), part.data_ptr(), stream()) < 0 and b"two samples" in lib().babe_last_error()


def _window():
    return torch.hann_window(2 * SIZE).cuda()


@pytest.mark.parametrize("e", [SIZE, OVERLAP, 60000])
def test_edge_masks_equal_prepare_smooth_mask(e):
    """The mask pair of an edge at sample e = the hard mask and BlindSampler.prepare_smooth_mask of it with the same table, bit for
    bit, into aligned rows and into rows that start off a 16-byte boundary; an edge inside the first `size` samples is refused."""
    from babe_amd._lib import lib, stream
    from babe_amd.testing.blind_bwe_sampler import BlindSampler
    want_mask = (torch.arange(L) < e).float().reshape(1, L)
    want_smooth = BlindSampler.prepare_smooth_mask(want_mask, SIZE)
    w = _window()
    for off in (0, 1):
        buf = torch.full((2, L + 4), -1.0, device="cuda")
        m, s = buf[0, off:off + L], buf[1, off:off + L]
        assert lib().babe_edge_masks(m.data_ptr(), s.data_ptr(), L, e, SIZE, w.data_ptr(), stream()) == 0
        assert torch.equal(m.cpu(), want_mask[0]) and torch.equal(s.cpu(), want_smooth[0])
        assert float(buf[:, :off].sum()) == -2.0 * off and float(buf[:, off + L:].sum()) == -2.0 * (4 - off)   # nothing around the rows
    only = torch.full((L,), -1.0, device="cuda")
    assert lib().babe_edge_masks(only.data_ptr(), None, L, e, 0, None, stream()) == 0 and torch.equal(only.cpu(), want_mask[0])
    assert lib().babe_edge_masks(only.data_ptr(), only.data_ptr(), L, SIZE - 1, SIZE, w.data_ptr(), stream()) < 0
    assert b"edge" in lib().babe_last_error()


def test_cut_scale_and_write_back_equal_their_torch_one_liners():
    from babe_amd._lib import lib, stream
    g = torch.Generator().manual_seed(9)
    src = torch.randn(1000 + 8, generator=g).cuda()
    s = torch.tensor([0.0371], device="cuda")
    for off in (0, 1):
        x = src[off:off + 1000]
        # a segment with a zero tail
        for n, length in ((1000, 1000), (999, 1000), (997, 1003), (1, 7), (0, 5)):
            dst = torch.full((length + 8,), -1.0, device="cuda")
            for doff in (0, 3):
                assert lib().babe_segment_cut(x.data_ptr(), n, dst.data_ptr() + 4 * doff, length, stream()) == 0
                want = torch.zeros(length, device="cuda")
                want[:n] = x[:n]
                assert torch.equal(dst[doff:doff + length], want) and float(dst[doff + length:].min()) == -1.0
        # the two scales: (a x) / s on the way in, x (s (1 / a)) on the way out
        out = torch.empty(1000, device="cuda")
        assert lib().babe_scale_dev(out.data_ptr(), x.data_ptr(), 1000, 0.1, s.data_ptr(), 0, stream()) == 0
        assert torch.equal(out, (0.1 * x) / s)
        assert lib().babe_scale_dev(out.data_ptr(), x.data_ptr(), 1000, float(np.float32(1.0) / np.float32(0.1)), s.data_ptr(), 1, stream()) == 0
        assert torch.equal(out, x * (s / 0.1))
        inplace = x.clone()
        assert lib().babe_scale_dev(inplace.data_ptr(), inplace.data_ptr(), 1000, 0.1, s.data_ptr(), 0, stream()) == 0
        assert torch.equal(inplace, (0.1 * x) / s)
    # a kept piece into the file: out[ix:ix + keep] = pred[:keep], the rest untouched
    file = torch.full((5000,), 7.0, device="cuda")
    want = file.clone()
    assert lib().babe_segment_cut(src.data_ptr(), 800, file.data_ptr() + 4 * 1234, 800, stream()) == 0
    want[1234:1234 + 800] = src[:800]
    assert torch.equal(file, want)


# ------------------------------------------------------------------------------------------------ the whole flow
def test_one_call_equals_the_python_flow_bit_for_bit(flows):
    """restore_recording_library, handed torch's standard deviation of the file, = restore_recording_complete(..., clip0=0) with
    the same blind segments and seed on the Python loop, in the restored file, the estimated filter and the blind step's
    restorations."""
    (out, filt, pred), (want, wfilt, wpred) = flows["lib"], flows["py"]
    assert out.shape == (LREC,) and filt.shape == (2, 5) and pred.shape == (2, L)
    assert torch.isfinite(out).all() and float(out.abs().max()) > 0
    assert torch.equal(filt, wfilt.reshape(filt.shape)), (filt, wfilt)
    assert torch.equal(pred, wpred), float((pred - wpred).abs().max())
    assert torch.equal(out, want), float((out - want).abs().max())
    from babe_amd._lib import lib
    starts, valid = (C.c_long * 3)(), (C.c_long * 3)()
    assert lib().babe_recording_plan(LREC, L, OVERLAP, 200, starts, valid, 3) == 3 and list(valid) == [L, L, LREC - starts[2]]
    assert starts[2] + valid[2] == LREC              # (no tail past the last written sample on this file)


def test_the_calls_own_standard_deviation(flows):
    """std_dev = NULL: the call measures the file itself (double sums, against torch's float reduction).  The scale may move by
    2 ulp before three sampling steps.  Measured once on this fixture (MI355X): the relative difference of the restored file to
    the run handed torch's value is 0 - the two standard deviations are the same float here - so the margin of 4x on it asserts
    equality."""
    out, want = flows["own"][0], flows["lib"][0]
    rel = float((out.double() - want.double()).norm() / want.double().norm())
    print(f"std_dev = NULL against torch's: relative difference of the restored file {rel:.3e}")
    assert torch.isfinite(out).all() and rel <= 4 * MEASURED_REL


MEASURED_REL = 0.0        # relative L2 difference measured on this fixture (see the test above)


def test_tail_past_the_last_written_sample_is_zero(world):
    """A file whose last segment is longer than segL (the walk truncates it): out past the last written sample is zero, here and
    in the Python flow, and the two agree."""
    from babe_amd._lib import lib
    hop = L - OVERLAP - 200
    n = hop + L + 150                                 # the last segment starts at hop with segL + 150 samples left: 150 are dropped
    starts, valid = (C.c_long * 2)(), (C.c_long * 2)()
    assert lib().babe_recording_plan(n, L, OVERLAP, 200, starts, valid, 2) == 2 and list(valid) == [L, L] and starts[1] == hop
    rec = world["rec"][:n].contiguous()
    s = rec.reshape(1, -1).std(-1)
    out = _library_flow(world, rec, [0], s)[0]
    assert out.shape == (n,) and float(out[hop + L:].abs().max()) == 0.0 and float(out[hop + L - 1].abs()) > 0
    want = _python_flow(world, rec, [0])[0]
    assert torch.equal(out, want)


def test_short_file_takes_the_one_segment_branch(world):
    """Lrec = 50000 < segL: one zero-padded segment for the blind step and for the restoration; = restore_recording_complete."""
    rec = world["rec"][:50000].contiguous()
    s = rec.reshape(1, -1).std(-1)
    out, filt, pred = _library_flow(world, rec, [0], s)
    want, wfilt, wpred = _python_flow(world, rec, [0])
    assert out.shape == (50000,) and torch.isfinite(out).all() and float(out.abs().max()) > 0
    assert torch.equal(filt, wfilt.reshape(filt.shape)) and torch.equal(pred, wpred) and torch.equal(out, want)


def test_restore_cli_mode_complete(world, tmp_path, monkeypatch):
    """python -m babe_amd.restore --mode complete --blind-segments 2 --seed 3 on a wav of the recording: --loop library (one
    babe_restore_recording call) and --loop python write the same bytes; --mode segments is another flow and another file."""
    import sys
    from scipy.io import wavfile
    import babe_amd.config as config
    from babe_amd import restore
    wav = str(tmp_path / "in.wav")
    wavfile.write(wav, FS, world["rec"].cpu().numpy())
    real = config.default_args
    monkeypatch.setattr(config, "default_args", lambda **k: real(**dict(k, Ns=NS)))
    outs = {}
    for tag, extra in (("lib", ["--mode", "complete", "--blind-segments", "2", "--loop", "library"]),
                       ("py", ["--mode", "complete", "--blind-segments", "2", "--loop", "python"]), ("seg", ["--loop", "library"])):
        monkeypatch.setattr(sys, "argv", ["restore", wav, str(tmp_path / tag), "--T", str(T), "--sample-rate", str(FS), "--audio-len", str(L),
                                          "--seed", "3"] + extra)
        restore.main()
        outs[tag] = open(str(tmp_path / tag / "in.wav"), "rb").read()
        assert os.path.exists(str(tmp_path / tag / "in.filter_data.pkl"))
    assert len(outs["lib"]) > 44 + 2 * LREC and outs["lib"] == outs["py"] and outs["lib"] != outs["seg"]


# ------------------------------------------------------------------------------------------------ the C host
def test_c_host_equals_the_ctypes_call_byte_for_byte(world, tmp_path):
    """examples/c_host/babe_restore_recording as a fresh child process on the 240000-sample recording = a ctypes
    babe_restore_recording call on the same model file with babe_edm_steps rows, the same window table, blind segments and seed
    (both sides measure the file's standard deviation themselves), in the restored file and the printed filter."""
    from babe_amd import model_file
    from babe_amd._cabi import RecordingDesc
    from babe_amd._lib import check, lib, ptr, stream
    from babe_amd.build import build_example
    from babe_amd.testing import model_c
    tmp = str(tmp_path)
    path = os.path.join(tmp, "small.babe")
    model_file.export(world["net"], world["args"], path)
    exe = build_example(out=os.path.join(tmp, "babe_restore_recording"), src="babe_restore_recording.c")
    rec = world["rec"]
    rec.cpu().numpy().tofile(os.path.join(tmp, "in.f32"))
    r = subprocess.run([exe, path, os.path.join(tmp, "in.f32"), os.path.join(tmp, "out.f32"), "--seed", "11", "--blind-segments", "2"],
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    x_c = np.fromfile(os.path.join(tmp, "out.f32"), np.float32)
    lines = r.stdout.split("\n")
    assert lines[0].startswith("fc_Hz ") and lines[1].startswith("A_dB ")
    f_c = np.array([[float(v) for v in ln.split()[1:]] for ln in lines[:2]], np.float32)

    model = model_c.LibraryModel(path)
    state = lib().babe_unet_state_create()
    try:
        d = RecordingDesc()
        d.eval = model.eval_desc(state)
        rows_b, t0, warm = model_c.edm_steps(model, T, 1.0)
        rows_k, _, _ = model_c.edm_steps(model, T, model.setting("tester.diff_params.Snoise"))
        d.T, d.t0, d.warm_start, d.steps_blind, d.steps_known = T, t0, int(warm), rows_b, rows_k
        d.n_blind = 2
        for j in range(2):
            d.blind_starts[j] = int(j * (LREC - L) / 1)
        init = _sampler(world)._init_params(1, rec.device)[0].contiguous()
        window = torch.tensor([0.5 - 0.5 * math.cos(2.0 * 3.14159265358979323846 * k / (2 * SIZE)) for k in range(2 * SIZE)],
                              dtype=torch.float64).float().cuda()
        d.init_params, d.target_std, d.overlap, d.discard_end = ptr(init), 0.1, int(0.25 * FS), 200
        d.inpaint_dc, d.dc_size, d.dc_window = 1, SIZE, ptr(window)
        need = lib().babe_recording_workspace_bytes(C.byref(d))
        assert need > 0, lib().babe_last_error()
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        out, filt = torch.empty(LREC, device="cuda"), torch.empty(2, 5, device="cuda")
        check(lib().babe_restore_recording(C.byref(d), ptr(rec), LREC, ptr(out), ptr(filt), None, 11, 0, ptr(ws), need, stream()), "restore_recording")
        torch.cuda.synchronize()
        assert x_c.shape == (LREC,) and np.isfinite(x_c).all() and x_c.tobytes() == out.cpu().numpy().tobytes()
        assert f_c.tobytes() == filt.cpu().numpy().tobytes()
    finally:
        lib().babe_unet_state_destroy(state)
        model.close()
