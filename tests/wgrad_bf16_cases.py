"""Case table and float64 references of the bf16-operand conv weight gradient (babe_conv_wgrad_bf16_rows), shared by the CPU
model test (test_wgrad_bf16_cases_cpu.py) and the GPU op test (test_gpu_wgrad_bf16.py).

Rounding model.  Both operands are rounded once to bf16 (8 significand bits, round to nearest even): a relative error uniform
in +-2^-9 per element, rms 2^-9 / sqrt(3) = 1.13e-3.  A product of two rounded values carries both, rms sqrt(2) * 1.13e-3 =
1.6e-3 if the error were independent of the mantissa; it is not (the relative step is largest just above a power of two), and
on Gaussian data the measured ratio |P_rounded - P| / |P| is 2.3e-3 to 2.4e-3, independent of the sum length because every term
of a sum carries its own independent error.  The CPU test pins that figure to [1.5e-3, 3.5e-3]; the GPU test's bars rest on it:
against the ROUNDED float64 reference only fp32 accumulation is left (the fp32 op's own 2e-5 bar), against the unrounded one the
error must lie between 5e-4 (the bf16 kernel really ran) and 1e-2 (4 x the model)."""
import torch

CASES = [  # B, Cin, Cout, F, T, KH, KW, dil
    # the nine of tests/test_gpu_wgrad.py
    (2, 16, 32, 20, 100, 5, 3, 1),
    (1, 32, 64, 16, 257, 5, 3, 2),
    (2, 40, 72, 30, 64, 5, 3, 7),
    (1, 8, 8, 130, 33, 5, 3, 64),
    (2, 48, 72, 9, 100, 1, 1, 1),
    (1, 2, 64, 12, 100, 5, 3, 1),
    (2, 64, 2, 12, 257, 5, 3, 2),
    (1, 96, 2, 8, 64, 1, 1, 1),
    (1, 256, 256, 7, 64, 5, 3, 4),
    # T shorter than one 16-position MFMA step, exactly one, one past it
    (1, 16, 16, 3, 5, 5, 3, 1),
    (1, 16, 16, 4, 16, 5, 3, 1),
    (2, 16, 16, 4, 17, 5, 3, 2),
    # one channel past a tile on both sides; F = 1
    (1, 33, 65, 1, 40, 5, 3, 1),
    (1, 33, 65, 6, 40, 1, 1, 1),
]
# 63 steps of one 1 x 1 channel tile: two chunks (32 + 31 steps), the boundary inside a frequency row; a ragged last quad
CHUNK_CASE = (2, 16, 16, 21, 132, 5, 3, 3)
ALL_CASES = CASES + [CHUNK_CASE]


def case_id(c):
    return f"B{c[0]}_ci{c[1]}_co{c[2]}_F{c[3]}_T{c[4]}_k{c[5]}{c[6]}_d{c[7]}"


def case_inputs(case):
    """The seeded operands of tests/test_gpu_wgrad.py for this case."""
    B, Cin, Cout, F, T, KH, KW, dil = case
    gen = torch.Generator().manual_seed(sum(case))
    x = torch.randn(B, Cin, F, T, generator=gen)
    g = torch.randn(B, Cout, F, T, generator=gen)
    return x, g


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _rows(x, g, KH, KW, dil, dtype=torch.float64):
    B, Cin = x.shape[:2]
    Cout = g.shape[1]
    out = []
    for b in range(B):
        out.append(torch.nn.grad.conv2d_weight(x[b:b + 1].to(dtype).cpu(), (Cout, Cin, KH, KW), g[b:b + 1].to(dtype).cpu(),
                                               padding=(dil * (KH // 2), KW // 2), dilation=(dil, 1)))
    return torch.stack(out)            # [B, Cout, Cin, KH, KW]


def ref_rows(x, g, KH, KW, dil):
    """float64 weight gradient per batch row of the operands as given."""
    return _rows(x, g, KH, KW, dil)


def ref_rows_bf16(x, g, KH, KW, dil):
    """float64 weight gradient per batch row of the operands rounded to bf16 (torch: round to nearest even)."""
    return _rows(x.float().bfloat16(), g.float().bfloat16(), KH, KW, dil)


def ref_rows_bf16_f32acc(x, g, KH, KW, dil):
    """The same in fp32 arithmetic: what fp32 accumulation of the rounded operands costs."""
    return _rows(x.float().bfloat16(), g.float().bfloat16(), KH, KW, dil, torch.float32)


TIE_LO, TIE_HI = 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8       # both halfway between two bf16 values: to even -> 1 and 1 + 2^-6


def tie_inputs(Cin=16, Cout=16, F=6, T=24, dil=1):
    """x alternates the two tie values (in a pattern that differs from row to row and channel to channel); g holds one 1.0 per
    output channel, so every entry of the weight gradient is a single rounded x value or 0: exact in any arithmetic."""
    i = torch.arange(Cin * F * T).reshape(1, Cin, F, T)
    x = torch.where((i * 7 // 3 + i // T) % 2 == 0, torch.tensor(TIE_LO), torch.tensor(TIE_HI)).float()
    assert set(x.unique().tolist()) == {TIE_LO, TIE_HI}
    g = torch.zeros(1, Cout, F, T)
    for co in range(Cout):
        g[0, co, (co * 5) % F, (co * 11) % T] = 1.0
    return x, g
