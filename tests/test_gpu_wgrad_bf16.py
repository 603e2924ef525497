"""The bf16-operand conv weight gradient (babe_conv_wgrad_bf16_rows, ops.conv_wgrad_rows(precision='bf16')) against float64 on
the CPU: against the operands rounded to bf16 at the fp32 op's own bar, against the unrounded operands inside the rounding
model's bracket (tests/wgrad_bf16_cases.py), determinism, row independence, views, the gate dot and ties.  Needs a MI355X."""
import pytest
import torch

from tests.wgrad_bf16_cases import ALL_CASES, CHUNK_CASE, case_id, case_inputs, ref_rows, ref_rows_bf16, rel, tie_inputs

pytestmark = pytest.mark.gpu
TOL = 2e-5            # tests/test_gpu_wgrad.py's bar: the same fp32 accumulation lengths


@pytest.mark.parametrize("case", ALL_CASES, ids=[case_id(c) for c in ALL_CASES])
def test_conv_wgrad_bf16_rows_vs_float64(case):
    from babe_amd import ops
    B, Cin, Cout, F, T, KH, KW, dil = case
    x, g = case_inputs(case)
    want = ref_rows(x, g, KH, KW, dil)
    want_r = ref_rows_bf16(x, g, KH, KW, dil)
    xc, gc = x.cuda(), g.cuda()
    n = ops.conv_wgrad_workspace(xc, gc, KH, KW, dil, precision="bf16")
    chunks = n / (B * Cout * Cin * KH * KW)
    assert chunks == int(chunks) and chunks >= 1
    if case == CHUNK_CASE:
        assert chunks >= 2, chunks
    rows = torch.empty(B, Cout * Cin * KH * KW, device="cuda")
    ops.conv_wgrad_rows(xc, gc, KH, KW, rows, dil=dil, precision="bf16")
    for b in range(B):
        got = rows[b].view(Cout, Cin, KH, KW)
        er, eu = rel(got, want_r[b]), rel(got, want[b])
        print(f"{case_id(case)} row {b}: vs rounded float64 {er:.3e}, vs unrounded float64 {eu:.3e}, chunks {int(chunks)}")
        assert er < TOL
        assert 5e-4 < eu < 1e-2
    again = torch.empty_like(rows)
    ops.conv_wgrad_rows(xc, gc, KH, KW, again, dil=dil, precision="bf16")
    assert torch.equal(rows, again)
    if B == 2:                          # a row does not depend on the other rows of the call
        one = torch.empty(1, rows.shape[1], device="cuda")
        ops.conv_wgrad_rows(x[1:].cuda(), g[1:].cuda(), KH, KW, one, dil=dil, precision="bf16")
        assert torch.equal(one[0], rows[1])


def test_precision_keyword_is_checked():
    from babe_amd import ops
    x, g = case_inputs(ALL_CASES[9])
    with pytest.raises(ValueError):
        ops.conv_wgrad_workspace(x.cuda(), g.cuda(), 5, 3, precision="fp16")


@pytest.mark.parametrize("T", [130, 132], ids=["T130_elementwise", "T132_16byte_rows"])
def test_conv_wgrad_bf16_two_source_strided_scaled_and_gate_dot(T):
    from babe_amd import ops
    gen = torch.Generator().manual_seed(11)
    B, C1, C2, Cout, F, dil = 2, 24, 40, 48, 18, 2
    big_x = torch.randn(B, C1, F + 9, T, generator=gen)
    x2 = torch.randn(B, C2, F, T, generator=gen)
    big_g = torch.randn(B, Cout + 4, F + 5, T, generator=gen)
    x, g = big_x[:, :, 4:4 + F, :], big_g[:, 2:2 + Cout, 5:, :]
    os_ = torch.rand(B, Cout, generator=gen) + 0.5
    w = torch.randn(Cout, C1 + C2, 5, 3, generator=gen)
    alpha, galpha = 0.7, 0.3
    P = ref_rows_bf16(torch.cat([x, x2], 1), g, 5, 3, dil)
    want = alpha * os_.double()[:, :, None, None, None] * P
    want_gate = galpha * (P * w.double()[None]).sum((2, 3, 4))

    def run(bx, bg):
        rows = torch.empty(B, Cout * (C1 + C2) * 15, device="cuda")
        dgate_big = torch.zeros(B, Cout + 10, device="cuda")
        dgate = dgate_big[:, 3:3 + Cout]
        ops.conv_wgrad_rows(bx.cuda()[:, :, 4:4 + F, :], bg.cuda()[:, 2:2 + Cout, 5:, :], 5, 3, rows, dil=dil, x2=x2.cuda(),
                            oscale=os_.cuda(), alpha=alpha, w=w.cuda(), dgate=dgate, galpha=galpha, precision="bf16")
        return rows, dgate_big

    rows, dgate_big = run(big_x, big_g)
    dgate = dgate_big[:, 3:3 + Cout]
    er, eg = rel(rows.view(want.shape), want), rel(dgate, want_gate)
    print(f"rows vs rounded float64 {er:.3e}, gate dot {eg:.3e}")
    assert er < TOL
    assert eg < TOL
    assert float(dgate_big[:, :3].abs().sum()) == 0 and float(dgate_big[:, 3 + Cout:].abs().sum()) == 0
    flat = torch.empty(rows.shape[1], device="cuda")
    ops.rows_sum(rows, flat)
    assert rel(flat, want.sum(0).reshape(-1)) < TOL
    # the zero padding is that of the VIEW: what lies beside it in memory is never read
    nan_x = torch.full_like(big_x, float("nan"))
    nan_x[:, :, 4:4 + F, :] = x
    nan_g = torch.full_like(big_g, float("nan"))
    nan_g[:, 2:2 + Cout, 5:, :] = g
    rows_n, dgate_n = run(nan_x, nan_g)
    assert bool(torch.isfinite(rows_n).all()) and bool(torch.isfinite(dgate_n).all())
    assert torch.equal(rows_n, rows) and torch.equal(dgate_n, dgate_big)


@pytest.mark.parametrize("T", [24, 70, 23], ids=["T24", "T70_two_steps_elementwise", "T23_elementwise"])
def test_ties_round_to_even_through_the_kernel(T):
    """Every entry of the result is one rounded x value (or 0): exact, so the kernel's convert must give 1 and 1 + 2^-6 for the
    two halfway inputs (truncation and round-half-up each miss one of them)."""
    from babe_amd import ops
    x, g = tie_inputs(T=T)
    want = ref_rows_bf16(x, g, 5, 3, 1)
    rows = torch.empty(1, 16 * 16 * 15, device="cuda")
    ops.conv_wgrad_rows(x.cuda(), g.cuda(), 5, 3, rows, precision="bf16")
    assert torch.equal(rows.cpu().double().view(want.shape), want)
