"""HIP CQT (four-step DFT on the MFMA conv kernel + LDS band FFTs) vs the oracle NSGT.  Needs a MI355X.
(The band, gather and spec_scale kernels per band and per clip on small designs, every band length and path: tests/test_gpu_cqt_bands.py.)"""
import pytest
import torch

from oracle.nsgt import CQT_nsgt as OracleCQT

pytestmark = pytest.mark.gpu


def rel(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


@pytest.fixture(scope="module", params=[(22050, 92092), (44100, 368368)])
def pair(request):
    from babe_amd.cqt import CQT_nsgt
    fs, L = request.param
    return CQT_nsgt(7, 64, "oct", ("kaiser", 1), fs, L, device="cuda"), OracleCQT(7, 64, "oct", ("kaiser", 1), fs, L, dtype=torch.float64)


def test_rfft_and_transpose(pair):
    hip, _ = pair
    L = hip.Ls
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, L, generator=g)
    spec = hip.fft.rfft(x.cuda())
    ref = torch.fft.rfft(x.double())
    got = torch.complex(spec[:, 0, : L // 2 + 1].double().cpu(), spec[:, 1, : L // 2 + 1].double().cpu())
    assert float((got - ref).abs().max() / ref.abs().max()) < 5e-6
    # transpose: <rfft x, G> == <x, rfft_T G>
    G = torch.zeros(2, 2, hip.fft.KX)
    G[:, :, : L // 2 + 1] = torch.randn(2, 2, L // 2 + 1, generator=g)
    xt = hip.fft.rfft_T(G.cuda())
    lhs = float((spec.double().cpu() * G.double()).sum())
    rhs = float((x.double() * xt.double().cpu()).sum())
    assert abs(lhs - rhs) < 2e-5 * (abs(lhs) + abs(rhs) + 1e3)


def test_fwd_bwd_hpf_vs_oracle(pair):
    hip, orc = pair
    L = hip.Ls
    g = torch.Generator().manual_seed(2)
    x = 0.1 * torch.randn(2, L, generator=g)
    co = hip.fwd_planar(x.cuda())
    ref = orc.fwd(x.double().unsqueeze(1))
    assert [c.shape[-1] for c in co] == [r.shape[-1] for r in ref]
    for c, r in zip(co, ref):
        got = torch.complex(c[:, 0].double().cpu(), c[:, 1].double().cpu())
        assert float((got - r.squeeze(1)).abs().max() / r.abs().max()) < 2e-5
    # synthesis of arbitrary coefficients
    cs = [torch.randn(2, 2, 64, T, generator=g) for T in hip.T_oct]
    y = hip.bwd_planar([c.cuda() for c in cs])
    yref = orc.bwd([torch.complex(c[:, 0].double(), c[:, 1].double()).unsqueeze(1) for c in cs]).squeeze(1)
    assert rel(y, yref) < 2e-5
    # perfect reconstruction == high-pass
    xr = hip.bwd_planar(co)
    xh = hip.apply_hpf_DC(x.cuda())
    assert rel(xh, orc.apply_hpf_DC(x.double())) < 2e-5
    assert rel(xr, xh) < 2e-5
    # reference-style complex API
    cl = hip.fwd(x.cuda().unsqueeze(1))
    assert cl[0].shape == (2, 1, 64, hip.T_oct[0]) and cl[0].is_complex()
    assert rel(hip.bwd(cl).squeeze(1), xh) < 2e-5


def test_adjoints(pair):
    hip, _ = pair
    L = hip.Ls
    g = torch.Generator().manual_seed(3)
    x = torch.randn(1, L, generator=g).cuda()
    G = [torch.randn(1, 2, 64, T, generator=g).cuda() for T in hip.T_oct]
    co = hip.fwd_planar(x)
    lhs = sum(float((c.double() * gg.double()).sum()) for c, gg in zip(co, G))
    rhs = float((x.double() * hip.fwd_adjoint(G).double()).sum())
    assert abs(lhs - rhs) < 1e-4 * (abs(lhs) + abs(rhs)) + 1e-3
    y = hip.bwd_planar(G)
    gy = torch.randn(1, L, generator=g).cuda()
    gco = hip.bwd_adjoint(gy)
    lhs = float((y.double() * gy.double()).sum())
    rhs = sum(float((c.double() * gg.double()).sum()) for c, gg in zip(gco, G))
    assert abs(lhs - rhs) < 1e-4 * (abs(lhs) + abs(rhs)) + 1e-3


def test_hip_vs_cqt_nsgt_pytorch_library(pair):
    """HIP CQT against outputs of the reference's real dependency, when tests/golden/cqt_lib.npz exists (written by
    tests/golden/make_cqt_golden.py where `import cqt_nsgt_pytorch` works; absent in this build: skipped, and the CQT stays
    'parity unpinned').  First suspect on failure: the mirrored-band synthesis convention, oracle/nsgt.py bwd."""
    import os
    import numpy as np
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cqt_lib.npz")
    if not os.path.exists(path):
        pytest.skip("tests/golden/cqt_lib.npz absent (cqt_nsgt_pytorch not available where the goldens are made)")
    hip, _ = pair
    z = np.load(path)
    L = hip.Ls
    fs = 22050 if L == 92092 else 44100
    tag, sub = f"{fs}_{L}", 8
    g = torch.Generator().manual_seed(int(z[f"{tag}.seed"]))
    x = (0.1 * torch.randn(2, 1, L, generator=g)).squeeze(1).cuda()
    co = hip.fwd_planar(x)
    for j, c in enumerate(co):
        got = torch.stack([c[:, 0], c[:, 1]], -1)[..., ::max(1, sub // 2), :]
        assert rel(got, torch.from_numpy(z[f"{tag}.fwd{j}"])) < 1e-4, f"fwd octave {j}"
    assert rel(hip.bwd_planar(co)[:, ::sub], torch.from_numpy(z[f"{tag}.bwd"])) < 1e-4
    assert rel(hip.apply_hpf_DC(x)[:, ::sub], torch.from_numpy(z[f"{tag}.hpf"])) < 1e-4


@pytest.mark.parametrize("L", [46046, 184184, 92092, 368368, 441000])
def test_length_L_fft_and_transpose_other_lengths(L):
    """The mixed-radix four-step FFT (csrc/fft_mixed.hip) picks its radices per length - 46046 = (2 7 13)(11 23), 184184 = (4 7 13)
    (2 11 23): config #5's segment, ... - and 441000 = 630 x 700 = (2 3 3 5 7)(4 5 5 7), the only one with radices 3 and 5.  All
    five are supported lengths (a ValueError fails): RealFFT must equal torch.fft.rfft and its transpose must be the adjoint.
    (Small and odd lengths, every bin and the transpose element by element: tests/test_gpu_fft.py.)"""
    from babe_amd.cqt import RealFFT
    fft = RealFFT(L, torch.device("cuda"))
    assert fft.mixed
    g = torch.Generator().manual_seed(L % 997)
    x = torch.randn(2, L, generator=g)
    spec = fft.rfft(x.cuda())
    ref = torch.fft.rfft(x.double())
    got = torch.complex(spec[:, 0, : L // 2 + 1].double().cpu(), spec[:, 1, : L // 2 + 1].double().cpu())
    err = float((got - ref).abs().max() / ref.abs().max())
    G = torch.zeros(2, 2, fft.KX)
    G[:, :, : L // 2 + 1] = torch.randn(2, 2, L // 2 + 1, generator=g)
    xt = fft.rfft_T(G.cuda())
    lhs = float((spec.double().cpu() * G.double()).sum())
    rhs = float((x.double() * xt.double().cpu()).sum())
    print(f"L={L}: N1 x N2 = {fft.N1} x {fft.N2}, mixed-radix {fft.mixed} ({getattr(fft, 'rad1', None)} / {getattr(fft, 'rad2', None)}), rfft err {err:.1e}")
    assert err < 5e-6
    assert abs(lhs - rhs) < 2e-5 * (abs(lhs) + abs(rhs) + 1e3)


@pytest.mark.parametrize("fs,L", [(22050, 92092), (44100, 368368), (16000, 184184)])
def test_library_plan_equals_the_python_sequenced_transform(fs, L, monkeypatch):
    """csrc/cqt_plan.hip (band design in C++, device tables, one C call per transform: babe_cqt_fwd / _bwd / _fwd_adjoint /
    _bwd_adjoint / _hpf) against this class sequencing the same kernels from the numpy design.  The two designs agree to a few
    float64 ulp (tests/test_cqt_plan_cpu.py), i.e. a 1-ulp float32 difference in < 1e-4 of the table entries: bar 1e-6 relative;
    fwd reads no table (analytic window) and must be bit-identical."""
    from babe_amd.cqt import CQT_nsgt
    monkeypatch.setenv("BABE_CQT_C", "0")                    # this class sequencing the kernels from the numpy design
    py = CQT_nsgt(7, 64, "oct", ("kaiser", 1), fs, L, device="cuda")
    monkeypatch.setenv("BABE_CQT_C", "1")                    # the library's plan (the default)
    cc = CQT_nsgt(7, 64, "oct", ("kaiser", 1), fs, L, device="cuda")
    monkeypatch.delenv("BABE_CQT_C")
    assert cc._plan and not py._plan
    g = torch.Generator().manual_seed(11)
    for B in (1, 3):
        x = (0.1 * torch.randn(B, L, generator=g)).cuda()
        c_py, c_cc = py.fwd_planar(x), cc.fwd_planar(x)
        assert all(torch.equal(a, b) for a, b in zip(c_py, c_cc)), "fwd: analytic window, same kernels, same order"
        gco = [torch.randn(c.shape, generator=g).cuda() for c in c_py]
        assert rel(cc.bwd_planar(gco), py.bwd_planar(gco)) < 1e-6
        assert rel(cc.fwd_adjoint(gco), py.fwd_adjoint(gco)) < 1e-6
        for a, b in zip(cc.bwd_adjoint(x), py.bwd_adjoint(x)):
            assert rel(a, b) < 1e-6
        assert rel(cc.apply_hpf_DC(x), py.apply_hpf_DC(x)) < 1e-6
    # and the reference API on top of the plan: bwd(fwd(x)) = apply_hpf_DC(x)
    x = (0.1 * torch.randn(2, 1, L, generator=g)).cuda()
    assert rel(cc.bwd(cc.fwd(x)).squeeze(1), cc.apply_hpf_DC(x.squeeze(1))) < 5e-5
