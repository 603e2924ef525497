"""Host side of the library-side sampling run (csrc/sample.hip, csrc/randn.hip, babe_amd/testing/sample_c.py): the Philox
definition, the schedule helper, argument validation and the struct mirrors.  No GPU."""
import ctypes as C
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def _lib():
    import __graft_entry__ as ge
    ge.build()
    from babe_amd._lib import lib
    return lib()


def _u32(*v):
    return (C.c_uint32 * len(v))(*v)


@pytest.mark.parametrize("ctr,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox4x32_10_known_answers(ctr, key, want):
    """babe_philox4x32 - the host statement of what the noise kernel computes - against the Random123 known answers."""
    L = _lib()
    c, k, o = _u32(*ctr), _u32(*key), _u32(0, 0, 0, 0)
    assert L.babe_philox4x32(C.cast(c, C.c_void_p), C.cast(k, C.c_void_p), C.cast(o, C.c_void_p)) == 0
    assert tuple(o) == want, [hex(v) for v in o]
    assert L.babe_philox4x32(None, None, None) < 0 and b"bad arguments" in L.babe_last_error()


def _edm(**over):
    from babe_amd.config import default_args
    from babe_amd.diff_params.edm import EDM
    dp = EDM(default_args())
    for k, v in over.items():
        setattr(dp, k, v)
    return dp


@pytest.mark.parametrize("over,order,start_sigma", [
    ({}, 2, None),
    ({}, 2, 0.05),
    ({"Schurn": 0}, 2, None),
    ({"Schurn": 0}, 2, 0.05),
    ({}, 1, None),
    ({}, 1, 0.05),
])
@pytest.mark.parametrize("T", [3, 35])
def test_edm_steps_agrees_with_the_python_schedule(over, order, start_sigma, T):
    """babe_edm_steps (double arithmetic) against sample_c.steps_from(EDM) (torch's float32): integer fields equal, floats within
    tol = (ro + 4) * 2^-23 relative - the float32 rounding of the schedule's base is amplified ro-fold by the power.
    T = 3 (the GPU fixture's schedule): every float field within tol as it stands.  T = 35 (the benchmark's schedule, where
    neighbouring noise levels are close and one of them lies next to sigma = 1): the noise levels t_hat and t_next within tol as
    they stand; a field DERIVED from a level carries the level's float32 error times the condition number of its formula, so
    its bound is tol times that number (never below 1): h = t_next - t_hat: (|t_next| + |t_hat|) / |h|; inject = sqrt(t_hat^2 -
    t^2), t_hat = (1 + gamma) t with gamma rounded to float32 on the torch side: 1 + 1 / (2 gamma + gamma^2); cskip: 2; cout, cin:
    1; cnoise = ln(sigma) / 4: 1 / |ln sigma|."""
    import math
    from babe_amd._cabi import SampleStep
    from babe_amd.testing import sample_c
    L = _lib()
    dp = _edm(**over)
    snoise = float(dp.Snoise)
    rows, t0, t = sample_c.steps_from(dp, T, order, start_sigma, snoise)
    got = (SampleStep * T)()
    g0 = C.c_float()
    rc = L.babe_edm_steps(got, C.cast(C.pointer(g0), C.c_void_p), T, order, dp.sigma_min, dp.sigma_max, dp.ro, dp.sigma_data, dp.Schurn,
                          dp.Stmin, dp.Stmax, snoise, -1.0 if start_sigma is None else start_sigma)
    assert rc == 0, L.babe_last_error()
    tol = (dp.ro + 4) * 2.0 ** -23
    close = lambda a, b, cond=1.0: abs(a - b) <= tol * max(1.0, cond) * abs(b)
    assert close(g0.value, t0), (g0.value, t0)
    for i in range(T):
        a, b = got[i], rows[i]
        assert a.heun == b.heun == int(order == 2 and i < T - 1), (i, a.heun, b.heun)
        cond = {"t_hat": 1.0, "t_next": 1.0, "h": 1.0, "inject": 1.0}
        if T != 3:
            g = b.t_hat / float(t[i]) - 1.0
            cond["h"] = (abs(b.t_next) + abs(b.t_hat)) / abs(b.h)
            cond["inject"] = 1.0 + 1.0 / (2 * g + g * g) if g > 0 else 1.0
        for f in ("t_hat", "inject", "t_next", "h"):
            assert close(getattr(a, f), getattr(b, f), cond[f]), (i, f, getattr(a, f), getattr(b, f))
        for nm, sig in (("c1", b.t_hat), ("c2", b.t_next)):
            ca, cb = getattr(a, nm), getattr(b, nm)
            if nm == "c2" and not b.heun:
                assert list(ca) == [0.0] * 4 and list(cb) == [0.0] * 4          # no second evaluation: left zero by both
                continue
            cc = [1.0] * 4 if T == 3 else [2.0, 1.0, 1.0, 1.0 / abs(math.log(sig))]
            for j in range(4):
                assert close(ca[j], cb[j], cc[j]), (i, nm, j, ca[j], cb[j])
    assert got[T - 1].t_next == 0.0 and got[T - 1].heun == 0 and rows[T - 1].t_next == 0.0
    if over.get("Schurn") == 0:
        assert all(rows[i].inject == 0.0 and got[i].inject == 0.0 for i in range(T))
    else:
        assert rows[0].inject > 0.0 and got[0].inject > 0.0                       # the churn is on in the default configuration
    assert L.babe_edm_steps(got, C.cast(C.pointer(g0), C.c_void_p), 1, 2, 1e-4, 1.0, 13.0, 0.06, 5.0, 0.0, 50.0, 1.0, -1.0) < 0
    assert L.babe_edm_steps(None, None, 3, 2, 1e-4, 1.0, 13.0, 0.06, 5.0, 0.0, 50.0, 1.0, -1.0) < 0


def test_sample_entry_points_refuse_bad_arguments_without_a_gpu():
    """Host-side validation of babe_sample_bwe / babe_sample_workspace_bytes / babe_randn (no GPU call is made on these paths): a
    NULL descriptor, T < 1, a NULL step table and a short workspace are each refused with a message."""
    from babe_amd._cabi import SampleDesc, SampleStep
    L = _lib()
    FAKE = 0x1000                                         # never dereferenced: every check below fails before a launch
    run = lambda d, ws, nbytes: L.babe_sample_bwe(d, FAKE, FAKE, FAKE, None, 0, 0, None, None, ws, nbytes, 1, None)
    assert run(None, FAKE, 1 << 40) < 0 and b"NULL descriptor" in L.babe_last_error()
    assert L.babe_sample_workspace_bytes(None, 1) == -1 and b"bad arguments" in L.babe_last_error()
    rows = (SampleStep * 3)()
    for r in rows:
        r.t_hat, r.t_next, r.h = 0.1, 0.0, -0.1
    d = SampleDesc()
    d.eval.L, d.eval.nfft = 92092, 1024
    d.T, d.steps = 0, rows
    assert run(C.byref(d), FAKE, 1 << 40) < 0 and b"T = 0" in L.babe_last_error()
    d.T, d.steps = 3, None
    assert run(C.byref(d), FAKE, 1 << 40) < 0 and b"NULL step table" in L.babe_last_error()
    d.steps = rows
    assert run(C.byref(d), FAKE, 4096) < 0 and b"workspace of 4096 bytes" in L.babe_last_error()
    assert run(C.byref(d), None, 0) < 0 and b"workspace" in L.babe_last_error()
    # enough for the run's own buffers, but no plans in the descriptor: refused as incomplete, still before any launch
    assert run(C.byref(d), FAKE, 1 << 40) < 0 and b"incomplete evaluation descriptor" in L.babe_last_error()
    assert L.babe_sample_workspace_bytes(C.byref(d), 1) == -1
    # the generator's entry points
    assert L.babe_randn(None, 8, 1, 8, 0, 0, 0, None) < 0 and b"bad arguments" in L.babe_last_error()
    assert L.babe_randn(FAKE, 4, 2, 8, 0, 0, 0, None) < 0 and b"row stride" in L.babe_last_error()
    assert L.babe_randn(FAKE + 2, 8, 1, 8, 0, 0, 0, None) < 0 and b"4-byte aligned" in L.babe_last_error()
    assert L.babe_rand_bits(FAKE, 8, 1, 8, 0, 1 << 32, 0, None) < 0 and b"counter words" in L.babe_last_error()
    assert L.babe_rand_bits(FAKE, 8, 1, 8, 0, 0, -1, None) < 0 and b"counter words" in L.babe_last_error()


def test_sample_structs_have_the_headers_layout(tmp_path):
    """babe_sample_step and babe_sample_desc by name (a mirror left out of _cabi.STRUCTS fails here), with the generated probe of
    tests/test_cabi_exports.py."""
    from babe_amd import _cabi
    from test_cabi_exports import _check_layout
    assert {"babe_sample_step", "babe_sample_desc"} <= set(_cabi.STRUCTS)
    _check_layout(tmp_path, {n: _cabi.STRUCTS[n] for n in ("babe_sample_step", "babe_sample_desc")})
    assert _cabi.STRUCTS["babe_sample_desc"].eval.size == C.sizeof(_cabi.STRUCTS["babe_eval_desc"])


def test_sampler_constructor_checks_loop_and_seed():
    from babe_amd.config import default_args
    from babe_amd.diff_params.edm import EDM
    from babe_amd.testing.blind_bwe_sampler import BlindSampler
    args = default_args()
    smp = BlindSampler(None, EDM(args), args)
    assert smp.loop == "python" and smp.seed is None and smp.noise_device == "cpu"
    assert BlindSampler(None, EDM(args), args, loop="library", seed=7).seed == 7
    with pytest.raises(ValueError, match="loop"):
        BlindSampler(None, EDM(args), args, loop="graph")
    with pytest.raises(ValueError, match="seed"):
        BlindSampler(None, EDM(args), args, noise_device="philox")
