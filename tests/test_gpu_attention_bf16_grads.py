"""Parameter-gradient kernels of training on the bf16 attention core, H = 8: the relative-position table and qk-bias gradients
(babe_attn_param_vjp_bf16) after the bf16 core's forward and input-VJP, against float64 autograd of the exact attention and
against the rounding model; the qk weight gradient on bf16 MFMA (babe_attn_qk_wgrad_bf16) against float64 of the rounded and of
the unrounded operands.  Bars and shapes: tests/attention_bf16_train_cases.py.  Needs a MI355X."""
import pytest
import torch

from tests import attention_bf16_train_cases as C
from tests.test_gpu_attention import ref_attn
from tests.test_gpu_attention_bf16 import make, run
from tests.test_gpu_attention_grads import nan_rows

pytestmark = pytest.mark.gpu
H = C.H


def rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-300))


def table_grads(qk, a, qb, bucket, emb, scale, dout):
    """The bf16 core's forward and input-VJP, then the table / bias gradients into NaN-banded strided rows."""
    from babe_amd import ops
    B, _, F, _ = a.shape
    out, lse, dqk, dv = run(qk, a, qb, bucket, emb, scale, dout)
    ebuf, demb = nan_rows(B, 32 * H)
    bbuf, dqkb = nan_rows(B, 2 * H * F)
    ops.attn_param_vjp(qk, a, out, lse, dout, dqk, scale, qk_bias=qb, bucket=bucket, emb=emb, demb_rows=demb, dqkb_rows=dqkb,
                       precision="bf16")
    torch.cuda.synchronize()
    return ebuf, demb, bbuf, dqkb, dqk, out


@pytest.mark.parametrize("F,T", C.GPU_SHAPES)
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("bias", [False, True])
def test_attn_param_vjp_bf16_vs_float64(F, T, B, bias):
    qk, a, qb, bucket, emb = make(B, F, T, True, bias=bias)
    scale = F ** -0.5
    dout = C.make_dout(a.shape).cuda()
    ebuf, demb, bbuf, dqkb, dqk, out = table_grads(qk, a, qb, bucket, emb, scale, dout)
    for buf in (ebuf, bbuf):                                   # the guard bands of the strided rows are untouched
        assert torch.isnan(buf[:, :3]).all() and torch.isnan(buf[:, -3:]).all()
    assert torch.isfinite(demb).all() and torch.isfinite(dqkb).all()
    # float64 autograd of the exact attention on the unrounded inputs, one batch row at a time
    want = []
    for b in range(B):
        e64 = emb.double().requires_grad_(True)
        o = ref_attn(qk[b:b + 1].double(), a[b:b + 1].double(), scale, None if qb is None else qb.double(), bucket, e64)
        ge, = torch.autograd.grad((o * dout[b:b + 1].double()).sum(), e64)
        want.append(ge)
    want = torch.stack(want)
    model = C.demb_model(qk, a, qb, bucket, emb, scale, dout, rounded=True)
    model_o = C.demb_model(qk, a, qb, bucket, emb, scale, dout, rounded=True, out=out)       # D from the forward's own output
    got = demb.reshape(B, 32, H)
    eb = rel(dqkb, dqk.double().sum(-1))                       # the row sum of the same dqk
    if T == 1:
        ee, em = float(got.abs().max()), float((got.double() - model).abs().max())
        print(f"F={F} T={T} B={B} bias={bias}: max |demb| {ee:.2e} (vs rounded model {em:.2e}), dqkb {eb:.2e}")
        assert ee <= C.BAR_DQK_T1
    else:
        ee, em, eo = C.rel_rows(got, want), C.rel_rows(got, model), C.rel_rows(got, model_o)
        print(f"F={F} T={T} B={B} bias={bias}: demb vs exact {ee:.2e}, vs rounded model {em:.2e} (with the forward's own output "
              f"{eo:.2e}), dqkb {eb:.2e}")
        assert ee <= C.BAR_DEMB
        assert em <= C.BAR_DEMB_VS_MODEL
        assert eo <= C.BAR_DEMB_VS_MODEL_OUT
    assert eb <= C.TOL_FP32_ACC
    reached = torch.zeros(32, dtype=torch.bool)
    reached[bucket.cpu().long()] = True
    if T == 8:
        assert not reached.all()
    assert (got[:, ~reached] == 0.0).all()                     # exactly 0.0 over the NaN pre-fill


@pytest.mark.parametrize("F,T", [(64, 33), (448, 64)])
def test_attn_param_vjp_bf16_is_deterministic_and_row_independent(F, T):
    """Two runs bit for bit, and row 1 of a B = 2 call equals the B = 1 call on that row (the clip lanes split rows between
    calls)."""
    qk, a, qb, bucket, emb = make(2, F, T, True, bias=True)
    scale = F ** -0.5
    dout = C.make_dout(a.shape).cuda()
    _, demb, _, dqkb, _, _ = table_grads(qk, a, qb, bucket, emb, scale, dout)
    _, demb2, _, dqkb2, _, _ = table_grads(qk, a, qb, bucket, emb, scale, dout)
    assert torch.equal(demb, demb2) and torch.equal(dqkb, dqkb2)
    _, demb1, _, dqkb1, _, _ = table_grads(qk[1:].contiguous(), a[1:].contiguous(), qb, bucket, emb, scale, dout[1:].contiguous())
    assert torch.equal(demb[1:], demb1) and torch.equal(dqkb[1:], dqkb1)


def test_attn_param_vjp_bf16_refuses_what_does_not_fit():
    """F = 448 with T = 4096 needs more LDS than a CU has: an argument error before anything is launched."""
    from babe_amd._lib import lib
    L = lib()
    fake = 0x10000                                            # refused before anything is dereferenced
    rc = L.babe_attn_param_vjp_bf16(fake, None, fake, fake, fake, 32, fake, fake, fake, fake, fake, fake, 256, None, 0, 1, H, 448,
                                    4096, 0.05, None)
    assert rc == -1 and b"LDS" in L.babe_last_error()
    rc = L.babe_attn_param_vjp_bf16(fake, None, fake, None, None, 0, fake, fake, fake, fake, fake, None, 0, None, 0, 1, H, 64, 8,
                                    0.1, None)
    assert rc == -1 and b"nothing to compute" in L.babe_last_error()
    rc = L.babe_attn_param_vjp_bf16(None, None, fake, fake, fake, 32, fake, fake, fake, fake, fake, fake, 256, None, 0, 1, H, 64, 8,
                                    0.1, None)
    assert rc == -1 and b"null" in L.babe_last_error()


@pytest.mark.parametrize("F,T,B", C.QK_SHAPES)
def test_attn_qk_wgrad_bf16_vs_float64(F, T, B):
    """T = 1, T not a multiple of 4, the K-split levels (F = 64) and the single-chunk ones; beta = 0 over a NaN-filled output,
    beta = 1 accumulation, two runs bit for bit."""
    from babe_amd import ops
    HF = H * F
    dqk, a1 = C.qk_operands(F, T, B, "cuda")
    rounded, exact = C.qk_product(dqk, a1, True), C.qk_product(dqk, a1, False)
    ws = ops.attn_qk_wgrad_workspace(B, HF, T, precision="bf16")
    assert (ws > 0) == (F == 64 and B * -(-T // 32) >= 16), ws          # the K-split cases report a workspace
    dW = torch.full((2 * HF, HF), float("nan"), device="cuda")
    ops.attn_qk_wgrad(dqk, a1, dW, precision="bf16")
    e_r, e_x = rel(dW, rounded), rel(dW, exact)
    dW2 = torch.full((2 * HF, HF), float("nan"), device="cuda")
    ops.attn_qk_wgrad(dqk, a1, dW2, precision="bf16")
    assert torch.equal(dW, dW2)
    del dW2
    base = torch.randn(2 * HF, HF, device="cuda")
    acc = base.clone()
    ops.attn_qk_wgrad(dqk, a1, acc, alpha=0.5, beta=1.0, precision="bf16")
    e1 = rel(acc, base.double() + 0.5 * rounded)
    print(f"F={F} T={T} B={B}: vs rounded operands {e_r:.2e} (beta=1 {e1:.2e}), vs unrounded {e_x:.2e}, workspace {ws}")
    assert e_r < C.TOL_FP32_ACC and e1 < C.TOL_FP32_ACC
    assert C.BAR_QK_MODEL[0] < e_x < C.BAR_QK_MODEL[1]        # the bf16 pipe ran


def test_attn_qk_wgrad_bf16_rounds_ties_to_even():
    from babe_amd import ops
    dqk, a1 = C.qk_tie_inputs()
    want = C.qk_product(dqk, a1, True)
    dW = torch.full(tuple(want.shape), float("nan"), device="cuda")
    ops.attn_qk_wgrad(dqk.cuda(), a1.cuda(), dW, precision="bf16")
    assert torch.equal(dW.double().cpu(), want)


def test_attn_qk_wgrad_bf16_refuses_shapes_outside_the_contract():
    from babe_amd import ops
    from babe_amd._lib import BabeHipError, lib, ptr
    L = lib()
    for HF in (256, 600, 4096):
        dqk, a1 = torch.zeros(1, 2 * HF, 4, device="cuda"), torch.zeros(1, HF, 4, device="cuda")
        dW = torch.zeros(2 * HF, HF, device="cuda")
        with pytest.raises(BabeHipError):
            ops.attn_qk_wgrad(dqk, a1, dW, precision="bf16")
        assert L.babe_attn_qk_wgrad_bf16(ptr(dqk), ptr(a1), ptr(dW), None, 1, HF, 4, 1.0, 0.0, None) == -1
        assert b"unsupported shape" in L.babe_last_error()
    assert L.babe_attn_qk_wgrad_bf16(None, None, None, None, 1, 512, 4, 1.0, 0.0, None) == -1
    assert b"null" in L.babe_last_error()
    # a K-split shape without its workspace
    B, HF, T = 3, 512, 1024
    assert L.babe_attn_qk_wgrad_bf16_workspace(B, HF, T) > 0
    dqk, a1 = torch.zeros(B, 2 * HF, T, device="cuda"), torch.zeros(B, HF, T, device="cuda")
    dW = torch.zeros(2 * HF, HF, device="cuda")
    assert L.babe_attn_qk_wgrad_bf16(ptr(dqk), ptr(a1), ptr(dW), None, B, HF, T, 1.0, 0.0, None) == -1
    assert b"workspace" in L.babe_last_error()
    with pytest.raises(ValueError):
        ops.attn_qk_wgrad(dqk, a1, dW, precision="fp16")
    torch.cuda.synchronize()
