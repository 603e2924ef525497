"""csrc/recording.hip without a GPU: the host-side walk babe_recording_plan against the walk of long_file.restore_file_AR restated
here, and the argument checks of babe_restore_recording / babe_recording_workspace_bytes / babe_score_eval that come before the
first device call (each refusal names the field)."""
import ctypes as C

import pytest

SEGL, OVERLAP, DISCARD = 92092, 5512, 200
HOP = SEGL - OVERLAP - DISCARD


def _walk(L, segL, overlap, discard_end):
    """[(start, samples of the file in the segment)] as restore_file_AR walks a file of L samples (long_file.py)."""
    if L <= segL:
        return [(0, L)]
    segs = [(0, segL)]
    ix = segL - overlap - discard_end
    while ix < L - segL - discard_end:
        segs.append((ix, segL))
        ix += segL - overlap - discard_end
    n = L - ix                                   # seg = y[ix:]
    segs.append((ix, n if n < segL else segL))   # (a longer rest is truncated to segL)
    return segs


def _lengths():
    Ls = {1, SEGL - 1, SEGL, SEGL + 1, SEGL + 200, SEGL + 201, 240000}
    for k in range(1, 5):
        Ls |= {k * HOP - 1, k * HOP, k * HOP + 1}
    return sorted(Ls)


@pytest.mark.parametrize("L", _lengths())
def test_plan_equals_the_walk_of_restore_file_AR(L):
    from babe_amd._lib import lib
    want = _walk(L, SEGL, OVERLAP, DISCARD)
    count = lib().babe_recording_plan(L, SEGL, OVERLAP, DISCARD, None, None, 0)
    assert count == len(want)
    starts, valid = (C.c_long * count)(), (C.c_long * count)()
    assert lib().babe_recording_plan(L, SEGL, OVERLAP, DISCARD, starts, valid, count) == count
    assert list(zip(starts, valid)) == want
    if count > 1:
        assert valid[count - 1] > OVERLAP            # the last segment always reaches past its known head
    # fewer entries than segments: the count is still returned and nothing past max_segments is written
    if count > 1:
        short = (C.c_long * count)(*([-7] * count))
        assert lib().babe_recording_plan(L, SEGL, OVERLAP, DISCARD, short, None, count - 1) == count
        assert short[count - 1] == -7 and list(short)[:count - 1] == [s for s, _ in want[:-1]]


def test_plan_refuses_a_walk_that_does_not_advance():
    from babe_amd._lib import lib
    for args in ((240000, SEGL, 0, DISCARD), (240000, SEGL, SEGL - DISCARD, DISCARD), (0, SEGL, OVERLAP, DISCARD),
                 (240000, SEGL, OVERLAP, -1)):
        assert lib().babe_recording_plan(*args, None, None, 0) == -1 and b"recording_plan" in lib().babe_last_error()


FAKE = 0x1000                                    # a non-NULL pointer that is never dereferenced: every call below is refused first


def _desc():
    """A descriptor that passes the driver's own checks (its evaluation part is empty: refused later, still before a device call)."""
    from babe_amd._cabi import RecordingDesc, SampleStep
    d = RecordingDesc()
    d.eval.L, d.eval.K = SEGL, 2
    d.T, d.t0, d.warm_start = 3, 0.05, 1
    rows = (SampleStep * 3)()
    d.steps_blind, d.steps_known = rows, rows
    d.n_blind = 2
    d.blind_starts[0], d.blind_starts[1] = 0, 40000
    d.init_params, d.target_std, d.overlap, d.discard_end = FAKE, 0.1, OVERLAP, DISCARD
    d.inpaint_dc, d.dc_size, d.dc_window = 1, 50, FAKE
    d._keep = rows
    return d


def _refused(d, field, Lrec=240000, rec=FAKE, out=FAKE, ws=FAKE, sizes=True):
    from babe_amd._lib import lib
    rc = lib().babe_restore_recording(C.byref(d) if d is not None else None, rec, Lrec, out, None, None, 3, 0, ws, 1 << 40, None)
    msg = lib().babe_last_error().decode()
    assert rc < 0 and "restore_recording" in msg and field in msg, (field, rc, msg)
    if sizes:
        assert lib().babe_recording_workspace_bytes(C.byref(d) if d is not None else None) == -1
        msg = lib().babe_last_error().decode()
        assert "recording_workspace_bytes" in msg and field in msg, (field, msg)


def test_driver_refuses_bad_arguments_before_the_first_device_call():
    from ctypes import POINTER, cast
    from babe_amd._cabi import SampleStep
    _refused(None, "NULL descriptor")
    for name in ("rec", "out", "ws"):
        _refused(_desc(), "NULL rec, out or ws", sizes=False, **{name: None})
    d = _desc()
    d.steps_blind = cast(None, POINTER(SampleStep))
    _refused(d, "steps_blind")
    d = _desc()
    d.steps_known = cast(None, POINTER(SampleStep))
    _refused(d, "steps_known")
    d = _desc()
    d.init_params = None
    _refused(d, "init_params")
    d = _desc()
    d.dc_window = None
    _refused(d, "dc_window")
    for n in (0, -1, 17):
        d = _desc()
        d.n_blind = n
        _refused(d, "n_blind")
    d = _desc()
    d.blind_starts[1] = 240000 - SEGL + 1
    _refused(d, "blind_starts[1]", sizes=False)
    d = _desc()
    d.blind_starts[0] = -1
    _refused(d, "blind_starts[0]", sizes=False)
    d = _desc()
    d.blind_starts[1] = 1                          # a file shorter than a segment has its one blind segment at 0
    _refused(d, "blind_starts[1]", Lrec=50000, sizes=False)
    for ov in (50, 49, 0):
        d = _desc()
        d.overlap = ov
        _refused(d, "overlap")
    for ov in (SEGL - DISCARD, SEGL):
        d = _desc()
        d.overlap = ov
        _refused(d, "overlap")
    # the descriptor's own fields pass: the (empty) evaluation part is what is refused next, still on the host
    from babe_amd._lib import lib
    assert lib().babe_recording_workspace_bytes(C.byref(_desc())) == -1 and b"eval_workspace_bytes" in lib().babe_last_error()


def test_score_eval_refuses_a_mask_with_blind_and_a_dc_mask_without_mask():
    from babe_amd._cabi import EvalDesc
    from babe_amd._lib import lib

    def call(**fields):
        d = EvalDesc()
        for name in ("unet_plan", "unet_state", "cqt_plan", "rff_freq", "film_W", "film_b", "env_inv", "tw4096"):
            setattr(d, name, FAKE)
        d.L, d.nfft, d.K, d.rff_n = SEGL, 4096, 2, 32
        d.emb_dim[0] = 64
        for k, v in fields.items():
            setattr(d, k, v)
        rc = lib().babe_score_eval(C.byref(d), FAKE, 0.1, 1.0, 1.0, 1.0, 0.0, FAKE, FAKE, FAKE, FAKE, FAKE, None, FAKE, 1 << 40, 1, None)
        return rc, lib().babe_last_error().decode()

    rc, msg = call(mask=FAKE, blind=1)
    assert rc < 0 and "mask with blind = 1" in msg
    rc, msg = call(dc_mask=FAKE, dc_y=FAKE)
    assert rc < 0 and "without mask" in msg
    rc, msg = call(mask=FAKE, dc_mask=FAKE)
    assert rc < 0 and "come together" in msg
    rc, msg = call(mask=FAKE, mask_bs=7)
    assert rc < 0 and "mask_bs" in msg
