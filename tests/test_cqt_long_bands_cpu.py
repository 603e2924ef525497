"""Band designs whose top octave has T = 8192 coefficients (segments above 8.5 s; csrc/cqt.hip: band_fft13_kernel), on the host:
the numpy design (babe_amd/cqt.py::design_bands), the library's (csrc/cqt_plan.hip: babe_cqt_design_create_ex with max_band = 8192)
and what each entry goes on refusing.  No GPU call is made.  The GPU side: tests/test_gpu_cqt_long_bands.py."""
import numpy as np
import pytest

from tests import cqt_cases as cc
from tests import test_cqt_plan_cpu as tp

# the small design of the long band: one octave of four 8192-point bands - one shorter than 4096 samples, one just above, one
# that reaches past L/2 - over every three-pass plan, at a length where the whole transform is cheap
LONG13 = dict(L=32768, N=(128, 256), numocts=8, binsoct=4, beta=1.0, T_oct=[64, 128, 256, 512, 1024, 2048, 4096, 8192],
              wrap_low=0, mirror_high=1, max_sources=3, M_eq_4=0, M_eq_T=0, kdeg=5)
LONG13_M_TOP = [3446, 4120, 4928, 5869]
LONG13_NWIN = 35838
ARGS = (float(cc.FS), LONG13["L"], LONG13["numocts"], LONG13["binsoct"], LONG13["beta"])


@pytest.fixture
def long13(monkeypatch):
    monkeypatch.setitem(cc.CASES, "long13", LONG13)
    return "long13"


def _refused(entry, *args):
    L = tp._lib()
    d = getattr(L, entry)(*args)
    if d:
        L.babe_cqt_design_destroy(d)
    return (not d), L.babe_last_error()


def test_numpy_design_of_the_small_long_band_case(long13):
    """design_bands reaches T = 8192 and the case has the properties the GPU tests rely on."""
    from babe_amd.cqt import design_bands, factor_len
    got = cc.properties(long13)
    assert got == {k: LONG13[k] for k in cc.PROPERTY_KEYS}, got
    d = design_bands(cc.FS, LONG13["L"], LONG13["numocts"], LONG13["binsoct"], LONG13["beta"])
    assert d["nwin"] == LONG13_NWIN and list(d["M"][-4:]) == LONG13_M_TOP and factor_len(LONG13["L"]) == LONG13["N"]
    assert d["M"][-4] < 4096 < d["M"][-3] and d["c"][-1] + d["M"][-1] - d["M"][-1] // 2 - 1 > LONG13["L"] // 2
    geo = cc.geometry(long13)                                   # the oracle's design: the same rasterisation
    assert geo.T_oct == LONG13["T_oct"] and geo.nwin == LONG13_NWIN and cc.max_sources(long13) == 3


def test_library_design_with_max_band_8192_equals_the_numpy_design(monkeypatch):
    """Table by table, the comparison of tests/test_cqt_plan_cpu.py, with the library's design made by the _ex entry; the
    workgroup table gives each 8192-point band a workgroup of its own, at the end."""
    L = tp._lib()
    monkeypatch.setattr(L, "babe_cqt_design_create", lambda *a: L.babe_cqt_design_create_ex(*a, 8192), raising=False)
    tp.test_library_design_equals_numpy_design(cc.FS, LONG13["L"], LONG13["numocts"], LONG13["binsoct"], LONG13["beta"])
    d = L.babe_cqt_design_create_ex(*ARGS, 8192)
    assert d, L.babe_last_error()
    try:
        wgf, wgc = tp._get(L, d, "wg_first", np.int32), tp._get(L, d, "wg_count", np.int32)
        assert list(wgf[-4:]) == [28, 29, 30, 31] and list(wgc[-4:]) == [1, 1, 1, 1] and len(wgf) == 15
        assert list(tp._get(L, d, "T_oct", np.int32)) == LONG13["T_oct"]
    finally:
        L.babe_cqt_design_destroy(d)


def test_refusals():
    ok, msg = _refused("babe_cqt_design_create_ex", *ARGS, 4096)
    assert ok and msg.startswith(b"cqt design:") and b"4096" in msg, msg
    ok, msg5 = _refused("babe_cqt_design_create", *ARGS)
    assert ok and msg5 == msg, (msg5, msg)                      # the five-argument entry IS _ex(..., 4096)
    ok, msg = _refused("babe_cqt_design_create_ex", float(cc.FS), 65536, 8, 4, 1.0, 8192)        # a 16384-point band
    assert ok and msg.startswith(b"cqt design:") and b"8192" in msg and b"4096" not in msg, msg
    ok, msg = _refused("babe_cqt_design_create_ex", *ARGS, 5000)
    assert ok and msg.startswith(b"cqt design:") and b"max_band" in msg and b"5000" in msg, msg
    ok, msg = _refused("babe_cqt_design_create_ex", 44100.0, 368368, 7, 64, 1.0, 16384)
    assert ok and msg.startswith(b"cqt design:") and b"max_band" in msg, msg


INT64 = ("M", "c", "T", "woff", "idx", "rowptr", "src", "nb", "nwin", "M_dc", "N1", "N2", "K2", "KX", "kdeg")
FLOAT64 = ("f", "Om", "g", "gdual", "Tw", "hpf", "kpoly")
INT32 = ("rad1", "rad2", "wg_first", "wg_count", "T_oct")


def test_reference_design_is_the_same_through_both_entries():
    """(44100, 368368, 7, 64): every table the design exports, bit for bit."""
    L = tp._lib()
    a = L.babe_cqt_design_create(44100.0, 368368, 7, 64, 1.0)
    b = L.babe_cqt_design_create_ex(44100.0, 368368, 7, 64, 1.0, 8192)
    assert a and b, L.babe_last_error()
    try:
        for names, dt in ((INT64, np.int64), (FLOAT64, np.float64), (INT32, np.int32)):
            for n in names:
                ta, tb = tp._get(L, a, n, dt), tp._get(L, b, n, dt)
                assert ta.size > 0 and ta.tobytes() == tb.tobytes(), n
        assert int(tp._get(L, a, "T_oct", np.int32).max()) == 4096
    finally:
        L.babe_cqt_design_destroy(a)
        L.babe_cqt_design_destroy(b)


@pytest.mark.parametrize("fs,Ls,M_max", [(48000, 384000, 4168), (44100, 736736, 7997)])
def test_long_segments_design(fs, Ls, M_max):
    from babe_amd.cqt import design_bands
    d = design_bands(fs, Ls)
    assert [int(d["T"][j * 64]) for j in range(7)] == [128, 256, 512, 1024, 2048, 4096, 8192] and int(d["M"].max()) == M_max
    L = tp._lib()
    p = L.babe_cqt_design_create_ex(float(fs), Ls, 7, 64, 1.0, 8192)
    assert p, L.babe_last_error()
    try:
        assert list(tp._get(L, p, "T_oct", np.int32)) == [128, 256, 512, 1024, 2048, 4096, 8192]
        assert np.array_equal(tp._get(L, p, "M", np.int64), d["M"]) and np.array_equal(tp._get(L, p, "c", np.int64), d["c"])
    finally:
        L.babe_cqt_design_destroy(p)
    ok, msg = _refused("babe_cqt_design_create", float(fs), Ls, 7, 64, 1.0)
    assert ok and b"4096" in msg, msg
