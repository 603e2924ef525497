"""The rounding model the bars of tests/test_gpu_wgrad_bf16.py rest on, on the CPU (no GPU needed): what rounding both operands
of the conv weight gradient once to bf16 costs against float64, what fp32 accumulation adds, and where ties go."""
import pytest
import torch

from tests.wgrad_bf16_cases import (ALL_CASES, TIE_HI, TIE_LO, case_id, case_inputs, ref_rows, ref_rows_bf16, ref_rows_bf16_f32acc,
                                    rel, tie_inputs)


@pytest.mark.parametrize("case", ALL_CASES, ids=[case_id(c) for c in ALL_CASES])
def test_rounding_model_and_fp32_accumulation(case):
    KH, KW, dil = case[5:]
    x, g = case_inputs(case)
    want = ref_rows(x, g, KH, KW, dil)
    rounded = ref_rows_bf16(x, g, KH, KW, dil)
    model = rel(rounded, want)
    acc = rel(ref_rows_bf16_f32acc(x, g, KH, KW, dil), rounded)
    print(f"{case_id(case)}: bf16 operands vs float64 {model:.3e}; fp32 accumulation of the rounded operands {acc:.3e}")
    assert 1.5e-3 < model < 3.5e-3
    # far below the 2e-5 bar of the op test and far below the rounding itself: the bar separates the two
    assert acc < 5e-6


def test_ties_round_to_even():
    x = torch.tensor([TIE_LO, TIE_HI])
    assert x.bfloat16().float().tolist() == [1.0, 1 + 2.0 ** -6]
    # (a truncating convert gives 1 and 1 + 2^-7, round-half-up 1 + 2^-7 and 1 + 2^-6)
    x, g = tie_inputs()
    P = ref_rows_bf16(x, g, 5, 3, 1)
    assert set(P.unique().tolist()) == {0.0, 1.0, 1 + 2.0 ** -6}
    assert float((P - ref_rows(x, g, 5, 3, 1)).abs().max()) == 2.0 ** -8
