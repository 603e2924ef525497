"""predict_bwe's 'cheby1' / 'biquad' / 'resample' / 'decimate' degradations, host side: coefficient preparation, refusals,
length rules, prepare_filter and the sampler's argument errors (tests/golden/make_degradation_golden.py).  No GPU needed."""
import os

import numpy as np
import pytest
import torch

G = os.path.join(os.path.dirname(__file__), "golden")


def load(name):
    return {k: np.asarray(v) for k, v in np.load(os.path.join(G, name)).items()}


def _iir_cases():
    d = {**load("degradation_ops_iir1k.npz"), **load("degradation_ops_iir3k.npz")}
    return d, sorted({int(k[5]) for k in d if k.startswith("cheby")})


def _args(ftype, fc=3000, order=6, Q=0.707, fs=2000, factor=1):
    from babe_amd.config import default_args
    from babe_amd.config import to_attr
    args = default_args(sample_rate=22050, audio_len=92092, T=3)
    args.tester.bandwidth_extension = to_attr(dict(filter=dict(type=ftype, fc=fc, order=order, beta=1, ripple=0.05,
                                                               biquad=dict(Q=Q), resample=dict(fs=fs)),
                                                   decimate=dict(factor=factor)))
    return args


def test_prepare_iir_is_bit_exact_with_lfilters_fp32_normalisation():
    from babe_amd.degrade import prepare_iir
    d, cases = _iir_cases()
    for i in cases:
        bn, an = prepare_iir(d[f"cheby{i}_b"], d[f"cheby{i}_a"])
        assert np.array_equal(bn.numpy(), d[f"cheby{i}_bn"]) and np.array_equal(an.numpy(), d[f"cheby{i}_an"]), i
    o = load("degradation_ops_other.npz")
    c = o["biquad_coef"]
    bn, an = prepare_iir(c[:3], c[3:])
    assert np.array_equal(bn.numpy(), o["biquad_bn"]) and np.array_equal(an.numpy(), o["biquad_an"])
    assert float(d["cheby2_radius"]) > 0.99                           # the radius-0.99 case is among the fixtures


@pytest.mark.parametrize("order,sr,fc", [(8, 44100, 1000), (10, 22050, 1000)])
def test_unstable_fp32_filters_are_refused_with_their_radius(order, sr, fc):
    from babe_amd.degrade import prepare_iir
    from babe_amd.utils.bandwidth_extension import get_cheby1_ba
    b, a = get_cheby1_ba(order, 0.05, 2 * fc / sr)
    with pytest.raises(ValueError, match=r"pole radius 1\.\d+"):
        prepare_iir(b, a)


def test_order_limit_and_length_mismatch_are_refused():
    from babe_amd.degrade import MAX_ORDER, prepare_iir
    a = np.poly(0.5 * np.ones(MAX_ORDER + 1))
    with pytest.raises(ValueError, match=str(MAX_ORDER)):
        prepare_iir(np.ones(MAX_ORDER + 2), a)
    with pytest.raises(ValueError, match="len"):
        prepare_iir([1.0, 0.5], [1.0, -0.5, 0.1])
    th = (np.arange(MAX_ORDER // 2) + 0.5) * np.pi / (MAX_ORDER // 2)
    poles = 0.9 * np.exp(1j * np.concatenate([th, -th]))
    bn, an = prepare_iir(np.ones(MAX_ORDER + 1), np.real(np.poly(poles)))          # order 16 at radius 0.9 is accepted
    assert an.numel() == MAX_ORDER + 1


def test_decimate_and_resample_length_rules():
    from babe_amd.degrade import decimated_length
    from babe_amd.resample import resampled_length
    from oracle.resample import resample as oracle_resample
    for L in (1, 2, 3, 10, 11, 92092, 368368):
        for f in (1, 2, 3, 5):
            assert decimated_length(L, f) == torch.zeros(L)[..., 0:-1:f].shape[-1], (L, f)
    for L in (1, 99, 1000, 5001):
        for factor in (22050 / 2000, 22050 / 4000, 44100 / 3000):
            assert resampled_length(L, int(100 * factor), 100) == oracle_resample(torch.zeros(1, L), int(100 * factor), 100).shape[-1]


def test_prepare_filter_matches_the_reference():
    from babe_amd.utils.bandwidth_extension import prepare_filter
    d, cases = _iir_cases()
    for i in cases:
        order, sr, fc, _ = d[f"cheby{i}_cfg"]
        b, a = prepare_filter(_args("cheby1", fc=float(fc), order=int(order)), float(sr))
        assert np.array_equal(b, d[f"cheby{i}_b"]) and np.array_equal(a, d[f"cheby{i}_a"]), i
    o = load("degradation_ops_other.npz")
    fc, sr, Q = o["biquad_cfg"]
    c6 = prepare_filter(_args("biquad", fc=float(fc), Q=float(Q)), float(sr))
    assert len(c6) == 6 and all(v.dtype == torch.float32 and v.dim() == 0 for v in c6)
    assert np.array_equal(torch.stack(list(c6)).numpy(), o["biquad_coef"])
    for i in range(2):
        f = prepare_filter(_args("resample", fs=int(o[f"resample{i}_fs"])), 22050)
        assert f == float(o[f"resample{i}_factor"])
    for i in range(2):
        args = _args("decimate", factor=int(o[f"decimate{i}_factor"]))
        assert prepare_filter(args, 22050) == int(o[f"decimate{i}_factor"])
        assert args.tester.bandwidth_extension.filter.resample.fs == int(o[f"decimate{i}_fs_written"])
    for t in ("cheby1filtfilt", "butter_fir", "cheby1_fir", "nonsense"):
        with pytest.raises(NotImplementedError):
            prepare_filter(_args(t), 22050)


class _NoNet:
    CQTransform = None


@pytest.mark.parametrize("ftype,filt", [("resample", 22050 / 2000), ("decimate", 2)])
def test_predict_bwe_resample_and_decimate_refuse_start_sigma_and_data_consistency(ftype, filt):
    from babe_amd.config import default_args
    from babe_amd.diff_params.edm import EDM
    from babe_amd.testing.blind_bwe_sampler import BlindSampler
    args = default_args(sample_rate=22050, audio_len=92092, T=3, start_sigma=0.05)
    y = torch.zeros(1, 100)
    with pytest.raises(ValueError, match="start_sigma"):
        BlindSampler(_NoNet(), EDM(args), args).predict_bwe(y, filt, ftype)
    args = default_args(sample_rate=22050, audio_len=92092, T=3, start_sigma="None")
    args.tester.posterior_sampling.data_consistency = True
    with pytest.raises(ValueError, match="data_consistency"):
        BlindSampler(_NoNet(), EDM(args), args).predict_bwe(y, filt, ftype)
    args.tester.posterior_sampling.data_consistency = False
    with pytest.raises(ValueError, match="samples"):                 # y of the wrong length
        BlindSampler(_NoNet(), EDM(args), args).predict_bwe(y, filt, ftype)
