"""CPU checks of training on the bf16 attention core: the float64 rounding models of tests/attention_bf16_train_cases.py against the
exact results (the table-gradient bar is 2x the model; the qk weight gradient's window brackets one rounding per operand), the
model's sum against float64 autograd, and the four entry points at the library boundary."""
import ctypes
import os
import re

import pytest
import torch

from tests import attention_bf16_train_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["babe_attn_param_vjp_bf16", "babe_attn_param_vjp_bf16_workspace", "babe_attn_qk_wgrad_bf16",
       "babe_attn_qk_wgrad_bf16_workspace"]


def _cases():
    for F, T in C.CPU_SHAPES:
        for bias in ((True,) if T == 1024 else (False, True)):          # the long level once: 2 x 8 x 1024 x 1024 scores
            yield F, T, bias


@pytest.mark.parametrize("F,T,bias", list(_cases()))
def test_demb_rounding_model_is_within_half_the_bar(F, T, bias):
    qk, a, qb, bucket, emb = C.make_cpu(2, F, T, True, bias=bias)
    dout = C.make_dout(a.shape)
    scale = F ** -0.5
    exact = C.demb_model(qk, a, qb, bucket, emb, scale, dout, rounded=False)
    model = C.demb_model(qk, a, qb, bucket, emb, scale, dout, rounded=True)
    e = C.rel_rows(model, exact)
    print(f"F={F} T={T} bias={bias}: rounded model vs exact, worst row {e:.2e}")
    assert e <= 0.5 * C.BAR_DEMB


def test_demb_model_at_one_key_is_zero():
    qk, a, qb, bucket, emb = C.make_cpu(2, 64, 1, True, bias=True)
    dout = C.make_dout(a.shape)
    for rounded in (False, True):
        d = C.demb_model(qk, a, qb, bucket, emb, 64 ** -0.5, dout, rounded)
        assert float(d.abs().max()) <= 0.5 * C.BAR_DQK_T1


def test_exact_demb_model_is_float64_autograd():
    """The closed form the model sums equals autograd through the torch restatement of the attention core."""
    from tests.test_gpu_attention import ref_attn
    F, T = 64, 37
    qk, a, qb, bucket, emb = C.make_cpu(2, F, T, True)             # (no qk bias: the model adds it in fp32, as the kernels do)
    dout = C.make_dout(a.shape)
    e64 = emb.double().requires_grad_(True)
    o = ref_attn(qk.double(), a.double(), F ** -0.5, None, bucket, e64)
    ge, = torch.autograd.grad((o * dout.double()).sum(), e64)
    exact = C.demb_model(qk, a, qb, bucket, emb, F ** -0.5, dout, rounded=False)
    assert C.rel_rows(exact.sum(0, keepdim=True), ge[None]) < 1e-12


@pytest.mark.parametrize("F,T,B", C.QK_MODEL_SHAPES)
def test_qk_wgrad_rounding_model_lies_in_the_window(F, T, B):
    dqk, a1 = C.qk_operands(F, T, B)
    e = float((C.qk_product(dqk, a1, True) - C.qk_product(dqk, a1, False)).norm() / C.qk_product(dqk, a1, False).norm())
    print(f"F={F} T={T} B={B}: bf16-rounded operands vs unrounded {e:.2e}")
    assert C.BAR_QK_MODEL[0] < e < C.BAR_QK_MODEL[1]


def test_qk_tie_inputs_tell_the_rounding_modes_apart():
    dqk, a1 = C.qk_tie_inputs()
    want = C.qk_product(dqk, a1, True)
    assert set(want.unique().tolist()) == {1.0, 1 + 2.0 ** -6}
    assert not torch.equal(want, C.qk_product(dqk, a1, False))


def _params(name):
    hdr = open(os.path.join(ROOT, "include", "babe_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"\b" + name + r"\s*\(([^()]*)\)\s*;", hdr)
    assert m, f"{name}: not declared in include/babe_hip.h"
    return [p.strip() for p in m.group(1).split(",")]


def test_the_four_entry_points_are_declared_bound_and_exported():
    import __graft_entry__ as ge
    from babe_amd import _cabi
    ge.build()
    L = ctypes.CDLL(os.path.join(ROOT, "babe_amd", "libbabe_hip.so"))
    for name in NEW:
        assert name in _cabi.SIGS, name
        assert len(_cabi.SIGS[name][1]) == len(_params(name)), name
        assert len(_params(name)) == len(_params(name.replace("_bf16", ""))), name          # the fp32 twin's arguments
        assert hasattr(L, name), name


def test_ops_refuse_an_unknown_precision():
    from babe_amd import ops
    t = torch.zeros(1)
    with pytest.raises(ValueError):
        ops.attn_qk_wgrad(t, t, t, precision="fp16")
    with pytest.raises(ValueError):
        ops.attn_param_vjp(t, t, t, t, t, t, 1.0, precision="bf16x3")


def test_qk_wgrad_bf16_workspace_follows_the_fp32_plan_without_a_gpu():
    """The chunk count depends on (HF, T, B) only and is the fp32 call's: the K-split levels (HF = 512) report a workspace of
    whole [2HF, HF] partial tiles, the wide levels none, shapes outside the contract -1."""
    from babe_amd._lib import lib
    L = lib()
    for B, HF, T in [(1, 512, 1), (3, 512, 8), (2, 512, 129), (3, 512, 1024), (2, 3584, 64), (1, 2560, 100)]:
        n = L.babe_attn_qk_wgrad_bf16_workspace(B, HF, T)
        assert n == L.babe_attn_qk_wgrad_workspace(B, HF, T) and n >= 0 and n % (2 * HF * HF) == 0, (B, HF, T, n)
    assert L.babe_attn_qk_wgrad_bf16_workspace(3, 512, 1024) > 0
    for HF in (256, 600, 4096):
        assert L.babe_attn_qk_wgrad_bf16_workspace(1, HF, 4) == -1
    assert L.babe_attn_param_vjp_bf16_workspace(2, 8, 100, 32) == 2 * 8 * 100 + 2 * 8 * 7 * 32
    assert L.babe_attn_param_vjp_bf16_workspace(2, 8, 100, 65) == -1
