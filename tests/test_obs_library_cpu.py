"""Host side of the known degradations on the library path (csrc/eval_geom.h, csrc/sample.hip, babe_amd/testing/model_c.py): the FIR
design helper against scipy, the IIR stability check against degrade.prepare_iir, every refusal of the observation model before
a launch, the mapping of the degrade.py objects onto the descriptor, and the struct mirrors.  No GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

FAKE = 0x1000                                             # never dereferenced: every call below is refused before a launch

# (numtaps, cutoff, width, fs, highpass)
FIRWIN_CASES = [(500, 1000, 1, 44100, False), (500, 3000, 1, 44100, False), (200, 5000, 1, 22050, False), (33, 2000, 300, 22050, False),
                (64, 3000, 10, 44100, False), (499, 1000, 1, 44100, True), (101, 4000, 50, 16000, True)]


def _lib():
    import __graft_entry__ as ge
    ge.build()
    from babe_amd._lib import lib
    return lib()


@pytest.mark.parametrize("numtaps,cutoff,width,fs,highpass", FIRWIN_CASES)
def test_firwin_kaiser_equals_scipy(numtaps, cutoff, width, fs, highpass):
    """babe_firwin_kaiser against scipy.signal.firwin(numtaps, cutoff, width=width, window="kaiser", fs=fs[, pass_zero="highpass"]):
    every tap within 1e-14 in double (the taps are at most 1 in size: a few double roundings of sin, I0 and the normalising sum);
    the float32 images differ in at most 2 taps per filter, by one ulp each."""
    from scipy.signal import firwin
    from babe_amd.testing import model_c
    _lib()
    kw = dict(pass_zero="highpass") if highpass else {}
    want = firwin(numtaps, cutoff, width=width, window="kaiser", fs=fs, **kw)
    got = model_c.firwin_kaiser(numtaps, cutoff, width, fs, highpass)
    assert got.shape == want.shape == (numtaps,) and got.dtype == np.float64
    err = np.abs(got - want).max()
    print(f"firwin {numtaps, cutoff, width, fs, highpass}: max |difference| = {err:.3e}, max |tap| = {np.abs(want).max():.3f}")
    assert np.abs(want).max() <= 1.0
    assert err <= 1e-14
    g32, w32 = got.astype(np.float32), want.astype(np.float32)
    differ = np.nonzero(g32 != w32)[0]
    assert differ.size <= 2
    for i in differ:
        assert g32[i] in (np.nextafter(w32[i], np.float32(np.inf)), np.nextafter(w32[i], np.float32(-np.inf)))


def test_firwin_kaiser_refuses_what_scipy_refuses():
    L = _lib()
    out = (C.c_double * 64)()
    p = C.cast(out, C.c_void_p)
    assert L.babe_firwin_kaiser(33, 2000.0, 300.0, 22050.0, 0, p) == 0
    assert L.babe_firwin_kaiser(32, 2000.0, 300.0, 22050.0, 1, p) < 0 and b"even" in L.babe_last_error()      # high-pass, even numtaps
    assert L.babe_firwin_kaiser(33, 0.0, 300.0, 22050.0, 0, p) < 0 and b"cutoff" in L.babe_last_error()
    assert L.babe_firwin_kaiser(33, 11025.0, 300.0, 22050.0, 0, p) < 0 and b"cutoff" in L.babe_last_error()
    assert L.babe_firwin_kaiser(0, 2000.0, 300.0, 22050.0, 0, p) < 0
    assert L.babe_firwin_kaiser(33, 2000.0, 0.0, 22050.0, 0, p) < 0
    assert L.babe_firwin_kaiser(33, 2000.0, 300.0, 22050.0, 0, None) < 0


def _iir_cases():
    from scipy.signal import cheby1, zpk2tf
    cases = {f"cheby1 order {n}": cheby1(n, 0.05, 0.5) for n in (2, 6, 16)}
    # the same order at a lower cut-off: stable in double, its float32 coefficients have a pole at radius 1.12
    cases["narrow order 16, unstable in float32"] = cheby1(16, 1.0, 0.3)
    # a biquad low-pass (the RBJ cookbook form design_biquad_lpf computes), fc = 3 kHz at 22050 Hz, Q = 0.707
    w0 = 2 * np.pi * 3000 / 22050
    al = np.sin(w0) / (2 * 0.707)
    cases["biquad"] = ([(1 - np.cos(w0)) / 2, 1 - np.cos(w0), (1 - np.cos(w0)) / 2], [1 + al, -2 * np.cos(w0), 1 - al])
    z, p = [-1.0, -1.0], [1.05 * np.exp(0.4j), 1.05 * np.exp(-0.4j)]
    cases["pole at radius 1.05"] = tuple(np.real(c) for c in zpk2tf(z, p, 1.0))
    cases["len(b) != len(a)"] = ([1.0, 0.5], [1.0, -0.5, 0.25])
    cases["order 17"] = (np.r_[1.0, np.zeros(17)], np.r_[1.0, np.zeros(16), 0.5])
    return cases


@pytest.mark.parametrize("name", ["cheby1 order 2", "cheby1 order 6", "cheby1 order 16", "biquad", "pole at radius 1.05",
                                  "len(b) != len(a)", "order 17", "narrow order 16, unstable in float32"])
def test_iir_check_decides_what_prepare_iir_decides(name):
    """babe_iir_check (step-down test in double on the float32 coefficients) accepts exactly where degrade.prepare_iir returns
    coefficients, and refuses where it raises.  The C call has one `order` for both arrays, so the unequal lengths are refused
    by the binding (model_c.iir_check) - a C host has no such pair to pass."""
    from babe_amd.degrade import prepare_iir
    from babe_amd.testing import model_c
    _lib()
    b, a = _iir_cases()[name]
    try:
        bn, an = prepare_iir(b, a)
        accepted = True
    except ValueError:
        accepted = False
    if accepted:
        ok, msg = model_c.iir_check(bn.numpy(), an.numpy())
    else:           # prepare_iir's own normalisation, where it got that far
        b32, a32 = np.asarray(b, dtype=np.float32), np.asarray(a, dtype=np.float32)
        ok, msg = model_c.iir_check(b32 / a32[0], a32 / a32[0])
    assert ok == accepted, (name, ok, accepted, msg)
    assert accepted == name.startswith(("cheby1", "biquad"))


def test_iir_check_refuses_bad_arguments():
    L = _lib()
    one = (C.c_float * 3)(1.0, 0.0, 0.0)
    two = (C.c_float * 3)(2.0, 0.0, 0.0)
    p = lambda v: C.cast(v, C.c_void_p)
    assert L.babe_iir_check(p(one), p(one), 2) == 0
    assert L.babe_iir_check(None, p(one), 2) < 0 and L.babe_iir_check(p(one), None, 2) < 0
    assert L.babe_iir_check(p(one), p(one), 0) < 0 and b"order" in L.babe_last_error()
    assert L.babe_iir_check(p(one), p(two), 2) < 0 and b"a[0]" in L.babe_last_error()


def _desc(**fields):
    from babe_amd._cabi import EvalDesc
    d = EvalDesc()
    d.L, d.nfft = 92092, 1024
    for k, v in fields.items():
        setattr(d, k, v)
    return d


def _refusals():
    from babe_amd._cabi import OBS_CLIP, OBS_FIR, OBS_IIR, OBS_MASK
    fir = dict(obs_kind=OBS_FIR, taps=FAKE, ntaps=33)
    iir = dict(obs_kind=OBS_IIR, b=FAKE, a=FAKE, order=6)
    msk = dict(obs_kind=OBS_MASK, obs_mask=FAKE)
    clip = dict(obs_kind=OBS_CLIP, clip_value=0.1)
    # name -> (descriptor fields, y given)
    return {
        "unknown kind 5": (dict(obs_kind=5), True),
        "unknown kind -1": (dict(obs_kind=-1), True),
        "NULL taps": (dict(fir, taps=None), True),
        "empty taps": (dict(fir, ntaps=0), True),
        "order 0": (dict(iir, order=0), True),
        "order 17": (dict(iir, order=17), True),
        "NULL b": (dict(iir, b=None), True),
        "NULL obs_mask": (dict(msk, obs_mask=None), True),
        "clip_value < 0": (dict(clip, clip_value=-0.5), True),
        "dc_classic with the clip": (dict(clip, dc_classic=1), True),
        "blind with a FIR": (dict(fir, blind=1), True),
        "blind with a clip": (dict(clip, blind=1), True),
        "mask with an IIR": (dict(iir, mask=FAKE), True),
        "mask with a mask": (dict(msk, mask=FAKE), True),
        "mask with a clip": (dict(clip, mask=FAKE), True),
        "no y with a FIR": (fir, False),
        "no y with a clip": (clip, False),
        "no y with the AR mask": (dict(mask=FAKE), False),
    }


@pytest.mark.parametrize("name", ["unknown kind 5", "unknown kind -1", "NULL taps", "empty taps", "order 0", "order 17", "NULL b",
                                  "NULL obs_mask", "clip_value < 0", "dc_classic with the clip", "blind with a FIR",
                                  "blind with a clip", "mask with an IIR", "mask with a mask", "mask with a clip", "no y with a FIR",
                                  "no y with a clip", "no y with the AR mask"])
def test_observation_model_refusals_without_a_gpu(name):
    """Every refusal of the observation model returns "bad descriptor" from babe_score_eval and from babe_sample_bwe before any
    launch (host-side validation: the pointers are never dereferenced, there is no GPU here)."""
    from babe_amd._cabi import SampleDesc, SampleStep
    L = _lib()
    fields, has_y = _refusals()[name]
    y = FAKE if has_y else None
    d = _desc(**fields)
    rc = L.babe_score_eval(C.byref(d), FAKE, 0.1, 1.0, 1.0, 1.0, 0.0, y, None, FAKE, FAKE, FAKE, None, FAKE, 1 << 40, 1, None)
    assert rc < 0 and b"score_eval: bad descriptor" in L.babe_last_error(), (name, L.babe_last_error())
    rows = (SampleStep * 3)()
    for r in rows:
        r.t_hat, r.t_next, r.h = 0.1, 0.0, -0.1
    s = SampleDesc()
    s.eval, s.T, s.steps = d, 3, rows
    rc = L.babe_sample_bwe(C.byref(s), y, FAKE, FAKE, None, 0, 0, None, None, FAKE, 1 << 40, 1, None)
    assert rc < 0 and b"sample_bwe: bad descriptor" in L.babe_last_error(), (name, L.babe_last_error())


def test_accepted_observation_models_reach_the_next_check():
    """The same descriptors without their defect pass the observation checks: the call then stops at the next one (no plans in
    the descriptor), still before a launch - so the refusals above are the observation model's, not an accident of the fixture."""
    from babe_amd._cabi import OBS_CLIP, OBS_FIR, OBS_IIR, OBS_MASK
    L = _lib()
    for fields, y in [(dict(obs_kind=OBS_FIR, taps=FAKE, ntaps=33), FAKE), (dict(obs_kind=OBS_FIR, taps=FAKE, ntaps=32, mask=FAKE), FAKE),
                      (dict(obs_kind=OBS_IIR, b=FAKE, a=FAKE, order=16, clamp=1, dc_classic=1), FAKE),
                      (dict(obs_kind=OBS_MASK, obs_mask=FAKE, obs_mask_bs=92092, dc_classic=1), FAKE),
                      (dict(obs_kind=OBS_CLIP, clip_value=0.0), FAKE), (dict(), None)]:
        d = _desc(**fields)
        rc = L.babe_score_eval(C.byref(d), FAKE, 0.1, 1.0, 1.0, 1.0, 0.0, y, None, None, FAKE, FAKE, None, FAKE, 1 << 40, 1, None)
        assert rc < 0 and b"incomplete evaluation descriptor" in L.babe_last_error(), (fields, L.babe_last_error())


def test_unconditional_run_refuses_a_warm_start():
    from babe_amd._cabi import SampleDesc, SampleStep
    L = _lib()
    rows = (SampleStep * 3)()
    s = SampleDesc()
    s.eval, s.T, s.steps, s.warm_start = _desc(), 3, rows, 1
    rc = L.babe_sample_bwe(C.byref(s), None, None, FAKE, None, 0, 0, None, None, FAKE, 1 << 40, 1, None)
    assert rc < 0 and b"warm_start without y" in L.babe_last_error()
    s.warm_start = 0                                   # a cold start passes that check and stops at the next one (no plans)
    rc = L.babe_sample_bwe(C.byref(s), None, None, FAKE, None, 0, 0, None, None, FAKE, 1 << 40, 1, None)
    assert rc < 0 and b"incomplete evaluation descriptor" in L.babe_last_error()


def test_recording_and_file_flows_keep_to_the_stft_kind():
    """babe_restore_recording / babe_restore_file (through their workspace queries, which make the same descriptor check) refuse a
    descriptor whose observation model is not the STFT filter, and one with dc_classic."""
    from babe_amd._cabi import OBS_FIR, FileDesc, RecordingDesc, SampleStep
    L = _lib()
    rows = (SampleStep * 3)()

    def rec(**fields):
        r = RecordingDesc()
        r.eval = _desc(K=1, **fields)
        r.T, r.steps_blind, r.steps_known, r.n_blind, r.init_params = 3, rows, rows, 1, FAKE
        r.target_std, r.overlap, r.discard_end = 0.1, 100, 0
        return r

    for fields in (dict(obs_kind=OBS_FIR, taps=FAKE, ntaps=33), dict(dc_classic=1)):
        r = rec(**fields)
        assert L.babe_recording_workspace_bytes(C.byref(r)) == -1 and b"BABE_OBS_STFT" in L.babe_last_error()
        assert L.babe_restore_recording(C.byref(r), FAKE, 200000, FAKE, None, None, 0, 0, FAKE, 1 << 40, None) < 0
        assert b"BABE_OBS_STFT" in L.babe_last_error()
        f = FileDesc()
        f.rec = r
        f.lengths[0] = f.lengths[1] = f.lengths[2] = 200000
        assert L.babe_restore_file_workspace_bytes(C.byref(f)) == -1 and b"BABE_OBS_STFT" in L.babe_last_error()
        assert L.babe_restore_file(C.byref(f), FAKE, 200000, FAKE, None, None, None, 0, 0, FAKE, 1 << 40, None) < 0
        assert b"BABE_OBS_STFT" in L.babe_last_error()
    # the STFT kind passes that check and stops at the next one (no plans)
    r = rec()
    assert L.babe_recording_workspace_bytes(C.byref(r)) == -1 and b"BABE_OBS_STFT" not in L.babe_last_error()


def test_struct_mirrors_have_the_new_fields_and_the_headers_layout(tmp_path):
    """The appended fields are in the mirrors, at gcc's offsets (the generated probe of tests/test_cabi_exports.py), the enum values
    of the header are those of babe_amd/_cabi.py, and a zeroed descriptor is the STFT kind with nothing set."""
    import re
    from babe_amd import _cabi
    from test_cabi_exports import ROOT, _check_layout
    ev = [f for f, _ in _cabi.EvalDesc._fields_]
    assert ev[-11:] == ["obs_kind", "taps", "ntaps", "b", "a", "order", "clamp", "obs_mask", "obs_mask_bs", "clip_value", "dc_classic"]
    assert ev[-12] == "dc_y"                                            # appended: nothing before them moved
    assert [f for f, _ in _cabi.SampleDesc._fields_][-1] == "skip_zero_inject"
    _check_layout(tmp_path, {n: _cabi.STRUCTS[n] for n in ("babe_eval_desc", "babe_sample_desc", "babe_recording_desc", "babe_file_desc")})
    hdr = open(os.path.join(ROOT, "include", "babe_hip.h")).read()
    for name in ("STFT", "FIR", "IIR", "MASK", "CLIP"):
        assert int(re.search(rf"BABE_OBS_{name} = (\d+)", hdr).group(1)) == getattr(_cabi, "OBS_" + name)
    d = _cabi.EvalDesc()
    assert d.obs_kind == _cabi.OBS_STFT == 0 and not d.taps and not d.dc_classic and _cabi.SampleDesc().skip_zero_inject == 0


def test_observe_maps_the_degradation_objects_onto_the_descriptor():
    """model_c.observe: kind and parameters per degrade.py class, blind off for a known degradation, everything reset by the next
    call, the tensors kept alive on the descriptor.  (CPU tensors stand in: observe only takes addresses.)"""
    import torch
    from babe_amd import _cabi, degrade
    from babe_amd.testing import model_c
    import babe_amd._lib as _l
    mp = pytest.MonkeyPatch()
    mp.setattr(_l, "ptr", lambda t: None if t is None else t.data_ptr())          # (the package's ptr insists on device tensors)
    try:
        d = _cabi.EvalDesc()
        d.blind = 1
        fir = degrade.FIRDegradation(torch.ones(33) / 33, "cpu")
        assert model_c.observe(d, fir) is d
        assert (d.obs_kind, d.taps, d.ntaps, d.blind, d.dc_classic) == (_cabi.OBS_FIR, fir.taps.data_ptr(), 33, 0, 0) and not d.mask
        iir = degrade.IIRDegradation([0.2, 0.2], [1.0, -0.5], clamp=True, device="cpu")
        model_c.observe(d, iir, dc_classic=True)
        assert (d.obs_kind, d.b, d.a, d.order, d.clamp, d.dc_classic) == (_cabi.OBS_IIR, iir.b.data_ptr(), iir.a.data_ptr(), 1, 1, 1)
        assert not d.taps and d.ntaps == 0
        m1 = degrade.MaskDegradation(torch.ones(100), "cpu")
        model_c.observe(d, m1)
        assert (d.obs_kind, d.obs_mask, d.obs_mask_bs, d.order, d.dc_classic) == (_cabi.OBS_MASK, m1.mask.data_ptr(), 0, 0, 0)
        m2 = degrade.MaskDegradation(torch.ones(2, 100), "cpu")
        model_c.observe(d, m2)
        assert (d.obs_mask, d.obs_mask_bs) == (m2.mask.data_ptr(), 100)
        model_c.observe(d, degrade.ClipDegradation(0.25))
        assert d.obs_kind == _cabi.OBS_CLIP and d.clip_value == 0.25 and not d.obs_mask
        mask = torch.ones(2, 100)
        model_c.observe(d, degrade.MaskMixDegradation(mask, fir))
        assert (d.obs_kind, d.mask, d.mask_bs, d.taps) == (_cabi.OBS_FIR, mask.data_ptr(), 100, fir.taps.data_ptr())
        assert any(t is mask for t in d._keep) and any(t is fir.taps for t in d._keep)
        model_c.observe(d, degrade.MaskMixDegradation(mask[:1], None))
        assert (d.obs_kind, d.mask_bs, d.blind) == (_cabi.OBS_STFT, 0, 0) and d.mask and not d.taps
        d.blind = 1
        model_c.observe(d, None)
        assert d.obs_kind == _cabi.OBS_STFT and not d.mask and d.blind == 1            # nothing known: blind is the caller's
        with pytest.raises(NotImplementedError):
            model_c.observe(d, degrade.DecimateDegradation(2, 100))
        with pytest.raises(NotImplementedError):
            model_c.observe(d, degrade.MaskMixDegradation(mask, iir))
    finally:
        mp.undo()
