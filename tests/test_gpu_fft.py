"""The length-L real FFT under every CQT call, element by element against float64 references at small sizes and on every path:
the mixed-radix kernel (csrc/fft_mixed.hip) through its C-ABI and through RealFFT, its complex form (BABE_FFT_REAL=0, in a child
process), the dense fallback (two (1,1) conv stages around babe_fft_twiddle_transpose), and the host-side refusals.  Cases and
references: tests/fft_cases.py (pinned on the CPU by tests/test_fft_cases_cpu.py).  Needs a MI355X."""
import json
import os
import subprocess
import sys

import pytest
import torch

from tests import fft_cases as fc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNS = fc.runs()
RUN_IDS = [f"{fc.case_id(c)}-K2={K2}" for c, K2 in RUNS]

# Dense fallback: an output is a sum of N1 or N2 products on the fp32 MFMA conv kernel instead of log N passes.  Measured
# against the float64 references on a MI355X over every case of test_dense_fallback (max over directions and batch rows):
#   BABE_FFT_MIXED=0  L = 210: 2.0e-7 (B = 1), 1.9e-7 (B = 4)   L = 2112: 4.0e-7, 4.4e-7
#   no switch         L = 323: 2.1e-7, 2.1e-7                     L = 1798: 2.5e-7, 4.5e-7
# The bar is four times the largest of them, 4.48e-7 (the factor covers the seed-to-seed spread of a max-norm).
DENSE_BAR = 4 * 4.48e-7
# babe_fft_twiddle_transpose: one complex multiply by a float32 table entry of modulus 1 (the reference multiplies by the same
# rounded entry in float64): two rounded products and one rounded sum per component, |error| <= 3 u (|a_r w_r| + |a_i w_i|)
# <= 3 sqrt(2) u |a| with u = 2^-24.
TWIDDLE_BAR = 3 * 2 ** 0.5 * 2.0 ** -24


def _assert_run(r, bar, what):
    print(f"{what} {r.get('case', r.get('L'))} K2/B={r.get('K2', r.get('B'))}: fwd {max(r['fwd']):.2e}  transpose {max(r['tr']):.2e}  "
          f"adjoint gap {r['gap']:.2e} (bar {r['gap_bar']:.2e})")
    assert all(e < bar for e in r["fwd"]), (what, "forward", r["fwd"])
    assert all(e < bar for e in r["tr"]), (what, "transpose", r["tr"])
    assert r["gap"] <= r["gap_bar"] * bar / fc.BAR, (what, "adjoint", r["gap"], r["gap_bar"])


# ----------------------------------------------------------------------------- 1. direct C-ABI cases
@pytest.mark.parametrize("c,K2", RUNS, ids=RUN_IDS)
def test_mixed_radix_cabi_forward_and_transpose(c, K2):
    """babe_rfft_mixed at one row of the table: all KX bins of the forward transform and every sample of the transpose within
    5e-6 of the float64 references (max|got - ref| / max|ref| per batch row), the adjoint identity without absolute slack, no
    byte outside any buffer read into the result or written."""
    _assert_run(fc.run_case(c, K2), fc.BAR, "mixed")


# ----------------------------------------------------------------------------- 2. batch independence, determinism
@pytest.mark.parametrize("name", ["14x15", "5x7", "30x462"])
def test_batch_rows_are_independent_and_calls_repeat_bit_for_bit(name):
    N1, N2, rad1, rad2 = fc.case_by_id(name)[:4]
    K2 = fc.k2_of(N1, N2)
    x, G = fc.inputs(N1 * N2, K2 * N1, 3, seed=77)
    for direction, src in ((0, x), (1, G)):
        full, rc = fc.mixed_call(src, N1, N2, K2, rad1, rad2, direction)
        again, rc2 = fc.mixed_call(src, N1, N2, K2, rad1, rad2, direction)
        assert rc == 0 and rc2 == 0 and not bool(torch.isnan(full).any())
        assert torch.equal(full, again), f"direction {direction}: two identical calls differ"
        for b in range(3):
            one, rc = fc.mixed_call(src[b:b + 1], N1, N2, K2, rad1, rad2, direction)
            assert rc == 0 and torch.equal(one[0], full[b]), f"direction {direction}: row {b} of B = 3 differs from its B = 1 call"


# ----------------------------------------------------------------------------- 3. RealFFT at small and odd lengths
@pytest.mark.parametrize("L", [6, 35, 210, 2002, 2112, 13860])
def test_realfft_small_and_odd_lengths(L):
    """Through factor_len and small_radices (2002 = 26 x 77 is the L % 4 == 2 length with an odd N2).  These lengths are
    supported: a ValueError is a failure."""
    from babe_amd.cqt import RealFFT
    fft = RealFFT(L, torch.device("cuda"))
    print(f"L={L}: N1 x N2 = {fft.N1} x {fft.N2}, radices {fft.rad1} / {fft.rad2}")
    assert fft.mixed
    _assert_run(fc.run_front_end(fft, 2, seed=L), fc.BAR, "RealFFT")


# ----------------------------------------------------------------------------- 4. the dense fallback
@pytest.mark.parametrize("B", [1, 4])
@pytest.mark.parametrize("L,switch", [(210, True), (2112, True), (323, False), (1798, False)])
def test_dense_fallback(L, switch, B, monkeypatch):
    """RealFFT._rfft / _rfft_T on the dense DFT stages: forced by BABE_FFT_MIXED=0, or taken with no switch at lengths whose
    factors (17 x 19, 31 x 58) are outside the radix set.  B = 1 and 4: the two weight packings switch at B < 4."""
    from babe_amd.cqt import RealFFT
    if switch:
        monkeypatch.setenv("BABE_FFT_MIXED", "0")
    fft = RealFFT(L, torch.device("cuda"))
    assert fft.mixed is False
    _assert_run(fc.run_front_end(fft, B, seed=L + B), DENSE_BAR, "dense")


@pytest.mark.parametrize("N1,N2", [(17, 19), (33, 70)])
def test_twiddle_transpose_both_directions(N1, N2):
    """babe_fft_twiddle_transpose against a float64 complex multiply and transpose; neither factor is a multiple of its 32 x 32
    tile, so the ragged tiles run on both axes.  in [B][2][N1][N2] -> out [B][2][N2][N1] times tw[k1][n2], and the adjoint."""
    from babe_amd._lib import lib, stream
    B = 2
    tw = fc.tables(N1, N2)[2]
    twc = torch.complex(tw[..., 0].double(), tw[..., 1].double())                  # the float32 entries, exactly
    g = torch.Generator().manual_seed(N1 * N2)
    a, b = torch.randn(B, 2, N1, N2, generator=g), torch.randn(B, 2, N2, N1, generator=g)
    cx = lambda t: torch.complex(t[:, 0].double(), t[:, 1].double())
    ref_f = (cx(a) * twc).transpose(1, 2)
    ref_t = cx(b).transpose(1, 2) * twc.conj()
    twd = fc.Guarded(tw.numel(), src=tw)
    got = []
    for src, adjoint in ((a, 0), (b, 1)):
        inp, out = fc.Guarded(src.numel(), src=src), fc.Guarded(src.numel(), canary=-3.0)
        rc = lib().babe_fft_twiddle_transpose(inp.mid.data_ptr(), out.mid.data_ptr(), twd.mid.data_ptr(), B, N1, N2, adjoint, stream())
        torch.cuda.synchronize()
        assert rc == 0 and out.canaries_intact() and inp.canaries_intact()
        shape = (B, 2, N2, N1) if adjoint == 0 else (B, 2, N1, N2)
        got.append(out.mid.cpu().reshape(shape))
    ef, et = fc.row_err(cx(got[0]), ref_f), fc.row_err(cx(got[1]), ref_t)
    print(f"twiddle_transpose {N1}x{N2}: forward {max(ef):.2e}  adjoint {max(et):.2e}")
    assert all(e < TWIDDLE_BAR for e in ef + et), (ef, et)
    lhs, rhs = float((got[0].double() * b.double()).sum()), float((a.double() * got[1].double()).sum())
    bar = TWIDDLE_BAR * (float(fc.planar(ref_f).norm()) * float(b.double().norm()) + float(a.double().norm()) * float(fc.planar(ref_t).norm()))
    assert abs(lhs - rhs) <= bar, (lhs, rhs, bar)


def test_dense_fallback_cqt_vs_oracle_workload_size(monkeypatch):
    """The whole CQT at a workload length with the length-L transform on the dense path: no library plan may exist under
    BABE_FFT_MIXED=0 (the plan only has the mixed-radix form), and fwd / bwd / apply_hpf_DC meet the oracle as
    tests/test_gpu_cqt.py::test_fwd_bwd_hpf_vs_oracle asks of the default path."""
    from babe_amd.cqt import CQT_nsgt
    from oracle.nsgt import CQT_nsgt as OracleCQT
    fs, L = 22050, 92092
    monkeypatch.setenv("BABE_FFT_MIXED", "0")
    hip = CQT_nsgt(7, 64, "oct", ("kaiser", 1), fs, L, device="cuda")
    assert hip._plan is None and hip.fft.mixed is False
    orc = OracleCQT(7, 64, "oct", ("kaiser", 1), fs, L, dtype=torch.float64)
    rel = lambda p, q: float((p.detach().double().cpu() - q.double()).norm() / (q.double().norm() + 1e-30))
    g = torch.Generator().manual_seed(2)
    x = 0.1 * torch.randn(2, L, generator=g)
    co = hip.fwd_planar(x.cuda())
    ref = orc.fwd(x.double().unsqueeze(1))
    assert [c.shape[-1] for c in co] == [r.shape[-1] for r in ref]
    for c, r in zip(co, ref):
        got = torch.complex(c[:, 0].double().cpu(), c[:, 1].double().cpu())
        assert float((got - r.squeeze(1)).abs().max() / r.abs().max()) < 2e-5
    cs = [torch.randn(2, 2, 64, T, generator=g) for T in hip.T_oct]
    y = hip.bwd_planar([c.cuda() for c in cs])
    yref = orc.bwd([torch.complex(c[:, 0].double(), c[:, 1].double()).unsqueeze(1) for c in cs]).squeeze(1)
    assert rel(y, yref) < 2e-5
    xh = hip.apply_hpf_DC(x.cuda())
    assert rel(xh, orc.apply_hpf_DC(x.double())) < 2e-5
    assert rel(hip.bwd_planar(co), xh.cpu()) < 2e-5


# ----------------------------------------------------------------------------- 5. the complex form
def test_complex_form_of_both_stages_in_a_child_process():
    """BABE_FFT_REAL=0 is read once per process, so the whole table runs in one fresh child (started before it touches the GPU)
    through tests/fft_cases.py; the parent asserts the same bars on the errors it prints."""
    env = dict(os.environ)
    env["BABE_FFT_REAL"] = "0"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fft_cases.py")], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and "FFT_CASES_DONE" in r.stdout, (r.returncode, r.stdout[-1000:], r.stderr[-3000:])
    got = [json.loads(ln[len("FFT_CASE "):]) for ln in r.stdout.splitlines() if ln.startswith("FFT_CASE ")]
    assert [(d["case"], d["K2"]) for d in got] == [(fc.case_id(c), K2) for c, K2 in RUNS]
    for d in got:
        _assert_run(d, fc.BAR, "complex-form")


# ----------------------------------------------------------------------------- 6. refusals
REFUSALS = {
    "radix 17": dict(N1=17, N2=4, rad1=(17,), rad2=(4,)),
    "product is not N": dict(N1=8, N2=16, rad1=(4, 4), rad2=(4, 4)),
    "seven radices": dict(N1=2, N2=128, rad1=(2,), rad2=(2,) * 7),
    "K2 = N2 + 1": dict(N1=8, N2=16, rad1=(4, 2), rad2=(4, 4), K2_arg=17),
    "K2 = 0": dict(N1=8, N2=16, rad1=(4, 2), rad2=(4, 4), K2_arg=0),
    "null work": dict(N1=8, N2=16, rad1=(4, 2), rad2=(4, 4), work=None),
    "168000 bytes of LDS": dict(N1=2, N2=1400, rad1=(2,), rad2=(4, 2, 5, 5, 7)),
}


@pytest.mark.parametrize("direction", [0, 1])
@pytest.mark.parametrize("name", list(REFUSALS))
def test_host_side_refusals_leave_the_output_untouched(name, direction):
    """Each is refused on the host with the argument error (BABE_ERR_ARG = -1); nothing is launched, the pre-filled output keeps
    every value."""
    from babe_amd._lib import lib
    r = dict(REFUSALS[name])
    N1, N2, rad1, rad2 = r.pop("N1"), r.pop("N2"), r.pop("rad1"), r.pop("rad2")
    K2 = fc.k2_of(N1, N2)
    x, G = fc.inputs(N1 * N2, K2 * N1, 2, seed=3)
    out, rc = fc.mixed_call(x if direction == 0 else G, N1, N2, K2, rad1, rad2, direction, raw=True, **r)
    assert rc == -1, (name, rc)
    assert lib().babe_last_error().startswith(b"rfft_mixed")
    assert bool((out == 7.0).all()), f"{name}: refused, yet the output buffer changed"
