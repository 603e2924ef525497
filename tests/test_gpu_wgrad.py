"""Training kernels (csrc/wgrad.hip) against float64 on the CPU: the conv weight gradient (torch.nn.grad.conv2d_weight) with
dilations, ragged T, two-source and strided inputs, the output scale and the FiLM gate dot; the per-channel GroupNorm * FiLM
reduction; the Linear backward.  Needs a MI355X."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
TOL = 2e-5


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def ref_rows(x, g, KH, KW, dil):
    B, Cin = x.shape[:2]
    Cout = g.shape[1]
    out = []
    for b in range(B):
        out.append(torch.nn.grad.conv2d_weight(x[b:b + 1].double().cpu(), (Cout, Cin, KH, KW), g[b:b + 1].double().cpu(),
                                               padding=(dil * (KH // 2), KW // 2), dilation=(dil, 1)))
    return torch.stack(out)            # [B, Cout, Cin, KH, KW]


CASES = [  # B, Cin, Cout, F, T, KH, KW, dil
    (2, 16, 32, 20, 100, 5, 3, 1),
    (1, 32, 64, 16, 257, 5, 3, 2),
    (2, 40, 72, 30, 64, 5, 3, 7),
    (1, 8, 8, 130, 33, 5, 3, 64),
    (2, 48, 72, 9, 100, 1, 1, 1),
    (1, 2, 64, 12, 100, 5, 3, 1),
    (2, 64, 2, 12, 257, 5, 3, 2),
    (1, 96, 2, 8, 64, 1, 1, 1),
    (1, 256, 256, 7, 64, 5, 3, 4),
]


@pytest.mark.parametrize("case", CASES, ids=[f"B{c[0]}_ci{c[1]}_co{c[2]}_F{c[3]}_T{c[4]}_k{c[5]}{c[6]}_d{c[7]}" for c in CASES])
def test_conv_wgrad_rows_vs_float64(case):
    from babe_amd import ops
    B, Cin, Cout, F, T, KH, KW, dil = case
    gen = torch.Generator().manual_seed(sum(case))
    x = torch.randn(B, Cin, F, T, generator=gen)
    g = torch.randn(B, Cout, F, T, generator=gen)
    want = ref_rows(x, g, KH, KW, dil)
    rows = torch.empty(B, Cout * Cin * KH * KW, device="cuda")
    ops.conv_wgrad_rows(x.cuda(), g.cuda(), KH, KW, rows, dil=dil)
    for b in range(B):
        assert rel(rows[b].view(Cout, Cin, KH, KW), want[b]) < TOL
    again = torch.empty_like(rows)
    ops.conv_wgrad_rows(x.cuda(), g.cuda(), KH, KW, again, dil=dil)
    assert torch.equal(rows, again)
    if B == 2:                          # a row does not depend on the other rows of the call
        one = torch.empty(1, rows.shape[1], device="cuda")
        ops.conv_wgrad_rows(x[1:].cuda(), g[1:].cuda(), KH, KW, one, dil=dil)
        assert torch.equal(one[0], rows[1])


def test_conv_wgrad_two_source_strided_scaled_and_gate_dot():
    from babe_amd import ops
    gen = torch.Generator().manual_seed(11)
    B, C1, C2, Cout, F, T, dil = 2, 24, 40, 48, 18, 130, 2
    big_x = torch.randn(B, C1, F + 9, T, generator=gen)
    x2 = torch.randn(B, C2, F, T, generator=gen)
    big_g = torch.randn(B, Cout + 4, F + 5, T, generator=gen)
    x, g = big_x[:, :, 4:4 + F, :], big_g[:, 2:2 + Cout, 5:, :]
    os_ = torch.rand(B, Cout, generator=gen) + 0.5
    w = torch.randn(Cout, C1 + C2, 5, 3, generator=gen)
    alpha, galpha = 0.7, 0.3
    P = ref_rows(torch.cat([x, x2], 1), g, 5, 3, dil)
    want = alpha * os_.double()[:, :, None, None, None] * P
    want_gate = galpha * (P * w.double()[None]).sum((2, 3, 4))
    rows = torch.empty(B, Cout * (C1 + C2) * 15, device="cuda")
    dgate_big = torch.zeros(B, Cout + 10, device="cuda")
    dgate = dgate_big[:, 3:3 + Cout]
    ops.conv_wgrad_rows(big_x.cuda()[:, :, 4:4 + F, :], big_g.cuda()[:, 2:2 + Cout, 5:, :], 5, 3, rows, dil=dil, x2=x2.cuda(),
                        oscale=os_.cuda(), alpha=alpha, w=w.cuda(), dgate=dgate, galpha=galpha)
    assert rel(rows.view(want.shape), want) < TOL
    assert rel(dgate, want_gate) < TOL
    assert float(dgate_big[:, :3].abs().sum()) == 0 and float(dgate_big[:, 3 + Cout:].abs().sum()) == 0
    # rows_sum: the fixed-order batch reduction
    flat = torch.empty(rows.shape[1], device="cuda")
    ops.rows_sum(rows, flat)
    assert rel(flat, want.sum(0).reshape(-1)) < TOL


def gelu_grad64(u):
    return 0.5 * (1 + torch.erf(u / math.sqrt(2))) + u * torch.exp(-0.5 * u * u) / math.sqrt(2 * math.pi)


def test_gn_param_grad_vs_float64():
    from babe_amd import ops
    gen = torch.Generator().manual_seed(3)
    B, C, F, T, G = 2, 32, 12, 100, 8
    z = torch.randn(B, C, F, T, generator=gen)
    da = torch.randn(B, C, F, T, generator=gen)
    gamma = 1 + 0.2 * torch.randn(C, generator=gen)
    film = torch.randn(B, C + 6, generator=gen)
    zc, filmc = z.cuda(), film.cuda()
    stats, scale = ops.gn_scale(zc, gamma.cuda(), filmc[:, 3:3 + C])
    dg = torch.empty(B, C, device="cuda")
    dfilm = torch.zeros(B, 2 * C, device="cuda")
    cs = 0.8
    ops.gn_param_grad(zc, da.cuda(), scale, stats, gamma.cuda(), filmc[:, 3:3 + C], dg, dfilm[:, C:], cs=cs)
    z64, sc64 = z.double(), scale.double().cpu()
    r = stats[:, :, 2].double().cpu().repeat_interleave(C // G, 1)
    ds = cs * (da.double() * gelu_grad64(z64 * sc64[:, :, None, None]) * z64).sum((2, 3))
    assert rel(dg, ds * (film[:, 3:3 + C].double() + 1) * r) < TOL
    assert rel(dfilm[:, C:], ds * gamma.double() * r) < TOL
    assert float(dfilm[:, :C].abs().sum()) == 0


@pytest.mark.parametrize("relu", [False, True])
def test_linear_bwd_vs_float64(relu):
    from babe_amd import ops
    gen = torch.Generator().manual_seed(4)
    B, K, J = 3, 256, 1000
    x = torch.randn(B, K, generator=gen)
    W = torch.randn(J, K, generator=gen) / 16
    y = torch.randn(B, J, generator=gen) if relu else None
    dy = torch.randn(B, J, generator=gen)
    dW, db, dx = (torch.empty(J, K, device="cuda"), torch.empty(J, device="cuda"), torch.empty(B, K, device="cuda"))
    ops.linear_bwd(dy.cuda(), x.cuda(), W.cuda(), dW, db, dx=dx, y=y.cuda() if relu else None)
    dp = dy.double() * ((y > 0).double() if relu else 1)
    assert rel(dW, dp.t() @ x.double()) < TOL
    assert rel(db, dp.sum(0)) < TOL
    assert rel(dx, dp @ W.double()) < TOL
