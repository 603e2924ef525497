"""The case table and the float64 stage references of tests/test_gpu_cqt_bands.py, pinned without a GPU: what every small design
reaches (band lengths, wrapped and mirrored bands, sources per bin, window form), the stage references composed against the oracle
NSGT and float64 autograd through it, and the record and CSR forms of the gather tables walked on the CPU."""
import numpy as np
import pytest
import torch

from tests import cqt_cases as cc

TOL = 1e-12
IDS = list(cc.CASES)


@pytest.mark.parametrize("case", IDS)
def test_properties_equal_the_table(case):
    got = cc.properties(case)
    for key in cc.PROPERTY_KEYS:
        assert got[key] == cc.CASES[case][key], (case, key, got[key], cc.CASES[case][key])


def test_the_cases_cover_every_band_length_and_every_path():
    Ts = set()
    for case in IDS:
        Ts |= set(cc.CASES[case]["T_oct"])
    assert Ts == {1 << l for l in range(2, 13)}, sorted(Ts)
    by = cc.CASES
    assert {1 << l for l in range(9, 13)} <= set(by["long"]["T_oct"])                # every three-pass plan
    assert {1 << l for l in range(2, 9)} <= set(by["short"]["T_oct"])                # every one- and two-pass plan
    assert by["tiny"]["wrap_low"] > 0 and all(by[c]["mirror_high"] > 0 for c in IDS)
    assert by["tiny"]["max_sources"] > 3 and by["short"]["max_sources"] > 3            # the CSR gather
    assert all(by[c]["max_sources"] <= 3 for c in ("long", "deg7", "table", "rec9"))   # the record gather
    assert by["deg7"]["kdeg"] == 7 and by["table"]["kdeg"] is None
    assert all(by[c]["kdeg"] == 5 for c in ("tiny", "short", "long", "rec9"))
    assert by["tiny"]["M_eq_T"] > 0 and by["short"]["M_eq_4"] > 0


@pytest.mark.parametrize("case", IDS)
def test_geometry_from_the_oracle_equals_the_design_the_kernels_run_on(case):
    from babe_amd.cqt import design_bands, factor_len, small_radices
    c, geo = cc.CASES[case], cc.geometry(case)
    d = design_bands(cc.FS, c["L"], c["numocts"], c["binsoct"], c["beta"])
    for key in ("M", "c", "T", "woff"):
        assert np.array_equal(getattr(geo, key), d[key]), key
    assert geo.nwin == d["nwin"] and geo.T_oct == c["T_oct"]
    N1, N2 = factor_len(c["L"])
    assert (N1, N2) == c["N"] and geo.KX == ((c["L"] // 2) // N1 + 1) * N1 and geo.KX > c["L"] // 2 + 1
    assert small_radices(N1) and small_radices(N2) and c["binsoct"] >= 2          # the library's plan exists
    assert cc.max_sources(case) == c["max_sources"]
    orc = cc.oracle(case)
    assert float(np.abs(geo.diag - orc.diag).max() / orc.diag.max()) < TOL
    assert float(np.abs(geo.hpf - orc.Hhpf_full.numpy()[: c["L"] // 2 + 1]).max()) < TOL


def _signal(case, B, salt):
    g = torch.Generator().manual_seed(cc.seed_of(case, salt))
    return torch.randn(B, cc.CASES[case]["L"], generator=g, dtype=torch.float64)


@pytest.mark.parametrize("case", IDS)
def test_analysis_reference_composes_to_the_oracle(case):
    x = _signal(case, 2, 1)
    spec = cc.signal_to_spec(case, x)
    spec[:, :, cc.CASES[case]["L"] // 2 + 1:] = float("nan")                       # the reference reads no bin above L/2
    assert cc.worst(cc.coef_band_err(cc.ref_analysis(case, spec, "fwd"), cc.oracle_fwd(case, x))) < TOL
    # adjoint of synthesis: float64 autograd through oracle.bwd
    assert cc.worst(cc.coef_band_err(cc.ref_analysis(case, spec, "bwd_adjoint"), cc.oracle_bwd_adjoint(case, x))) < TOL


@pytest.mark.parametrize("case", IDS)
def test_synthesis_and_gather_references_compose_to_the_oracle(case):
    L = cc.CASES[case]["L"]
    co = [c.double() for c in cc.rand_coefs(case, 2, cc.seed_of(case, 2))]
    spec = cc.ref_gather(case, cc.ref_synthesis(case, co, "bwd"), 2.0 / L)
    assert bool((spec[:, :, L // 2 + 1:] == 0).all())
    assert cc.worst(cc.clip_err(cc.spec_to_signal(case, spec), cc.oracle_bwd(case, co))) < TOL
    # the same through irfft: the weights 1/L at DC and Nyquist, 2/L between, on the un-scaled gather
    half = cc.ref_gather(case, cc.ref_synthesis(case, co, "bwd"), 1.0)[:, :, : L // 2 + 1]
    # (the gather holds P[n] + conj(P[L-n]) between, and P alone at the two ends, where irfft takes the real part once)
    Z = torch.complex(half[:, 0], half[:, 1])
    Z[:, 0], Z[:, -1] = 2 * Z[:, 0].real, 2 * Z[:, -1].real
    assert cc.worst(cc.clip_err(torch.fft.irfft(Z, n=L, dim=-1), cc.oracle_bwd(case, co))) < TOL
    # adjoint of analysis: float64 autograd through oracle.fwd
    spec = cc.ref_gather(case, cc.ref_synthesis(case, co, "fwd_adjoint"), 1.0)
    assert cc.worst(cc.clip_err(cc.spec_to_signal(case, spec), cc.oracle_fwd_adjoint(case, co))) < TOL


@pytest.mark.parametrize("case", IDS)
def test_spec_scale_reference_composes_to_the_oracle_high_pass(case):
    geo = cc.geometry(case)
    x = _signal(case, 2, 3)
    spec = cc.signal_to_spec(case, x)
    out = cc.ref_spec_scale(case, spec, torch.from_numpy(geo.hpf * geo.irfft_w))
    assert bool((out[:, :, geo.L // 2 + 1:] == 0).all())
    assert cc.worst(cc.clip_err(cc.spec_to_signal(case, out), cc.oracle(case).apply_hpf_DC(x))) < TOL
    two = cc.ref_spec_scale(case, spec, None, 0.5, 3.0 * spec, 0.25)
    assert float((two[:, :, : geo.L // 2 + 1] - 1.25 * spec[:, :, : geo.L // 2 + 1]).abs().max()) < TOL * float(spec.abs().max())


@pytest.mark.parametrize("case", IDS)
def test_perfect_reconstruction_of_the_references(case):
    """bwd(fwd(x)) == apply_hpf_DC(x) through the stage references alone."""
    L = cc.CASES[case]["L"]
    x = _signal(case, 1, 4)
    co = cc.ref_analysis(case, cc.signal_to_spec(case, x), "fwd")
    y = cc.spec_to_signal(case, cc.ref_gather(case, cc.ref_synthesis(case, co, "bwd"), 2.0 / L))
    assert cc.worst(cc.clip_err(y, cc.oracle(case).apply_hpf_DC(x))) < TOL


# ----------------------------------------------------------------------------- the gather tables, walked on the CPU
def _design(case):
    from babe_amd.cqt import design_bands
    c = cc.CASES[case]
    return design_bands(cc.FS, c["L"], c["numocts"], c["binsoct"], c["beta"])


def _rec_table(d, L):
    """The record table exactly as CQT_nsgt.__init__ builds it; None when a bin has more than three sources."""
    rp, sr = np.asarray(d["rowptr"]), np.asarray(d["src"], dtype=np.int64)
    cnt = np.diff(rp)
    if cnt.max() > 3:
        return None
    rec = np.zeros((L // 2 + 1, 4), dtype=np.int64)
    for e in range(3):
        has = cnt > e
        rec[has, e] = sr[rp[:-1][has] + e]
    rec[:, 3] = cnt
    return rec.astype(np.int32)


def _walk(case, bs, sources):
    """sources(n) -> int32 entries of bin n (sign bit = conjugate), summed as gather_kernel / gather_rec_kernel do."""
    geo = cc.geometry(case)
    v = bs.double().numpy()
    v = v[..., 0] + 1j * v[..., 1]
    out = torch.zeros(bs.shape[0], 2, geo.KX, dtype=torch.float64)
    for n in range(geo.L // 2 + 1):
        acc = np.zeros(bs.shape[0], dtype=np.complex128)
        for s in sources(n):
            e = int(s) & 0x7FFFFFFF
            acc += np.conj(v[:, e]) if int(s) < 0 else v[:, e]
        out[:, 0, n], out[:, 1, n] = torch.from_numpy(acc.real), torch.from_numpy(acc.imag)
    return out


@pytest.mark.parametrize("case", ["long", "deg7", "rec9"])
def test_record_table_reproduces_the_gather_reference(case):
    d = _design(case)
    rec = _rec_table(d, cc.CASES[case]["L"])
    assert rec is not None and rec[:, 3].max() == cc.CASES[case]["max_sources"] <= 3
    bs = cc.rand_bs(case, 1, cc.seed_of(case, 5))
    got = _walk(case, bs, lambda n: rec[n, : rec[n, 3]])
    assert cc.worst(cc.clip_err(got, cc.ref_gather(case, bs, 1.0), planar_axis=1)) < TOL


@pytest.mark.parametrize("case", ["tiny", "short"])
def test_no_record_table_above_three_sources_and_the_csr_reproduces_the_reference(case):
    d = _design(case)
    assert cc.CASES[case]["max_sources"] > 3 and _rec_table(d, cc.CASES[case]["L"]) is None
    rp = np.asarray(d["rowptr"])
    src = np.asarray(d["src"], dtype=np.int64).astype(np.int32)                      # as the class uploads it
    bs = cc.rand_bs(case, 2, cc.seed_of(case, 5))
    got = _walk(case, bs, lambda n: src[rp[n]: rp[n + 1]])
    assert cc.worst(cc.clip_err(got, cc.ref_gather(case, bs, 1.0), planar_axis=1)) < TOL


# ----------------------------------------------------------------------------- the error measures
def test_the_band_measures_see_one_wrong_element_of_a_short_band():
    case = "short"
    geo = cc.geometry(case)
    ref = [c.double() for c in cc.rand_coefs(case, 2, 9)]
    bad = [r.clone() for r in ref]
    bad[0][1, 0, 3, 2] += 2 * cc.BAR * float(torch.hypot(ref[0][1, 0, 3], ref[0][1, 1, 3]).max())    # 4-point band 3 of clip 1
    e = cc.coef_band_err(bad, ref)
    assert e.shape == (2, geo.nb) and e[1, 3] > cc.BAR and np.count_nonzero(e) == 1
    bad[1][0, 1, 0, 0] = float("nan")
    assert np.isnan(cc.worst(cc.coef_band_err(bad, ref)))
    bs = cc.rand_bs(case, 2, 10).double()
    wrong = bs.clone()
    k = 2
    wrong[0, geo.woff[k] + geo.M[k] - 1, 1] += 2 * cc.BAR * float(torch.hypot(bs[0, geo.woff[k]: geo.woff[k] + geo.M[k], 0],
                                                                                bs[0, geo.woff[k]: geo.woff[k] + geo.M[k], 1]).max())
    e = cc.bs_band_err(case, wrong, bs)
    assert e.shape == (2, geo.nb) and e[0, k] > cc.BAR and np.count_nonzero(e) == 1
    assert np.isnan(cc.clip_err(torch.full((2, 5), float("nan")), torch.ones(2, 5))).all()
