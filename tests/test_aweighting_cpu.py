"""A-weighted training loss, host side: the pre-emphasis filter design against the reference's own taps
(tests/golden/aweighting.npz, written by tests/golden/make_aweighting_golden.py from utils/training_utils.py:71-122) and what
EDM builds from diff_params.aweighting.  No GPU work."""
import os

import numpy as np
import pytest
import torch

from babe_amd.config import default_args, to_attr
from babe_amd.diff_params.edm import EDM
from babe_amd.utils.training_utils import FIRFilter

FILTERS = {"aw_44100_101": dict(filter_type="aw", fs=44100), "aw_22050_101": dict(filter_type="aw", fs=22050),
           "aw_16000_51": dict(filter_type="aw", fs=16000, ntaps=51), "hp": dict(filter_type="hp"), "fd": dict(filter_type="fd")}


def fixture():
    return np.load(os.path.join(os.path.dirname(__file__), "golden", "aweighting.npz"))


def test_edm_builds_the_aweighting_filter():
    args = default_args()
    args.diff_params.aweighting = to_attr(dict(use_aweighting=True, ntaps=101))
    edm = EDM(args)
    assert isinstance(edm.AW, FIRFilter) and edm.AW.filter_type == "aw" and edm.AW.fs == 44100
    assert edm.AW.taps.shape == (101,) and edm.AW.taps.dtype == torch.float32
    assert torch.equal(edm.AW.taps, torch.from_numpy(fixture()["taps_aw_44100_101"]))


@pytest.mark.parametrize("name", ["edm_aweighting", "PD_edm_tapehiss"])
def test_edm_accepts_the_reference_aweighted_diff_params(name):
    """The two conf/diff_params files of the reference that set use_aweighting (stored as settings in the fixture)."""
    import yaml
    args = default_args(sample_rate=22050)
    args.diff_params = to_attr(yaml.safe_load(str(fixture()["conf_" + name])))
    assert args.diff_params.aweighting.use_aweighting is True
    edm = EDM(args)
    assert torch.equal(edm.AW.taps, torch.from_numpy(fixture()["taps_aw_22050_101"]))


@pytest.mark.parametrize("name", sorted(FILTERS))
def test_taps_equal_the_reference(name):
    """Both sides are the float32 rounding of the same float64 scipy computation."""
    f = FIRFilter(**FILTERS[name])
    want = torch.from_numpy(fixture()["taps_" + name])
    assert f.taps.dtype == torch.float32 and f.taps.dim() == 1
    assert torch.equal(f.taps, want), float((f.taps - want).abs().max())


def test_the_asymmetric_taps_are_not_flipped():
    assert FIRFilter("hp", coef=0.85).taps.tolist() == pytest.approx([1.0, -0.85, 0.0])
    assert FIRFilter("fd", coef=0.85).taps.tolist() == pytest.approx([1.0, 0.0, -0.85])
    assert FIRFilter().filter_type == "hp" and FIRFilter().ntaps == 101 and FIRFilter().fs == 44100


def test_even_ntaps_raises():
    for ft in ("hp", "fd", "aw"):
        with pytest.raises(ValueError):
            FIRFilter(ft, ntaps=100)


def test_aweighting_off_builds_no_filter():
    args = default_args()
    assert args.diff_params.aweighting.use_aweighting is False
    assert EDM(args).AW is None
    del args.diff_params["aweighting"]
    assert EDM(args).AW is None


def test_no_cpu_fallback():
    from babe_amd.stft import fir_sqerr
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        FIRFilter("hp")(torch.zeros(1, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fir_sqerr(torch.zeros(1, 8), torch.zeros(1, 8), torch.ones(3))


def test_fixture_is_self_consistent():
    """The recorded err2 is (A-weighting FIR of (stub(input, cnoise) - target))**2 in the F.conv1d(padding=K//2) convention: what
    the GPU tests compare the kernels with."""
    import torch.nn.functional as F
    g = fixture()
    a, b = (float(v) for v in g["stub"])
    w = torch.from_numpy(g["taps_aw_22050_101"]).double()
    for tag in ("long", "short"):
        t = lambda k: torch.from_numpy(g[f"{tag}_{k}"])
        d = (a * t("input") + b * t("cnoise") - t("target")).double()
        ew = F.conv1d(d[:, None], w[None, None], padding=50)[:, 0]
        assert float((ew ** 2 - t("err2")).abs().max()) <= 3e-6 * float((ew ** 2).max())
