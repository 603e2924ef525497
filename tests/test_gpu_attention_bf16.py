"""The bf16 time-attention kernels (csrc/attention_bf16.hip: babe_attn_fwd_bf16 / babe_attn_vjp_bf16) against the exact float64
attention on the unrounded inputs, under the bars of tests/attention_bf16_cases.py (which the CPU test ties to a rounding model):
every tiling edge of the kernels, ragged T, B = 1 and 2, relative bias on, and off with the qk bias; large logits, determinism
across runs and streams, the refusals.  Needs a MI355X."""
import ctypes

import pytest
import torch

from tests import attention_bf16_cases as ac

pytestmark = pytest.mark.gpu
H = ac.H


def make(B, F, T, rel_pos, bias=False, amp=1.0):
    return tuple(None if t is None else t.cuda() for t in ac.make_cpu(B, F, T, rel_pos, bias, amp))


def run(qk, a, qb, bucket, emb, scale, dout=None):
    from babe_amd import ops
    B, Hh, F, T = a.shape
    out = torch.full_like(a, float("nan"))                    # an element the kernel leaves out shows
    lse = torch.full((B, Hh, T), float("nan"), device=a.device)
    ops.attn_fwd(qk, a, out, lse, scale, qk_bias=qb, bucket=bucket, emb=emb, precision="bf16")
    if dout is None:
        return out, lse
    dqk, dv = torch.full_like(qk, float("nan")), torch.full_like(a, float("nan"))
    ops.attn_vjp(qk, a, out, lse, dout, dqk, dv, scale, qk_bias=qb, bucket=bucket, emb=emb, precision="bf16")
    return out, lse, dqk, dv


@pytest.mark.parametrize("F,T", ac.GPU_SHAPES)
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("rel_pos", [True, False])
def test_attention_bf16_fwd_vjp_vs_float64(F, T, B, rel_pos):
    qk, a, qb, bucket, emb = make(B, F, T, rel_pos, bias=not rel_pos)
    scale = F ** -0.5
    dout = ac.make_dout(a.shape).cuda()
    out, lse, dqk, dv = run(qk, a, qb, bucket, emb, scale, dout)
    torch.cuda.synchronize()
    exact = ac.model(qk, a, qb, bucket, emb, scale, dout, rounded=False)
    errs = ac.errors((out, dqk, dv), exact)
    print(f"F={F} T={T} B={B} rel_pos={rel_pos}: " + ", ".join(f"{k} {w:.2e}" + (f" (column {c:.2e})" if c is not None else "")
                                                               for k, (w, c) in errs.items()))
    for t in (out, lse, dqk, dv):
        assert torch.isfinite(t).all()
    ac.check(errs)
    # lse is fp32 arithmetic on scores of bf16-rounded operands: a score moves by about |S| * 2^-9
    x = qk.double() if qb is None else qk.double() + qb.double()[None, :, None]
    x = x.reshape(B, H, 2, F, T)
    s = torch.einsum("bhfn,bhfm->bhnm", x[:, :, 0], x[:, :, 1])
    if bucket is not None:
        idx = torch.arange(T, device="cuda")[None, :] - torch.arange(T, device="cuda")[:, None] + T - 1
        s = s + emb.double()[bucket.long()[idx]].permute(2, 0, 1)[None]
    assert (lse.double() - torch.logsumexp(s * scale, -1)).abs().max() < 2e-2


def test_attention_bf16_large_logits_stay_finite_and_convex():
    """The case of test_attention_large_logits_stay_finite (scores near +-80).  bf16 rounding of Q and K moves such scores by
    about 0.15, so no match to float64 is asked: every output is finite and every out[f][n] lies within the range of V[f][:],
    widened by 1 % of max |V| - softmax convexity, which holds at any precision."""
    F, T = 320, 100
    qk, a, qb, bucket, emb = make(1, F, T, True, amp=1.0)
    scale = F ** -0.5
    qk = qk.view(1, H, 2, F, T)
    q, k = qk[:, :, 0].double(), qk[:, :, 1].double()
    smax = float(torch.einsum("bhfn,bhfm->bhnm", q, k).abs().max()) * scale
    qk[:, :, 0] *= 80.0 / smax
    qk = qk.reshape(1, 2 * H * F, T).contiguous()
    dout = ac.make_dout(a.shape, seed=3).cuda()
    out, lse, dqk, dv = run(qk, a, qb, bucket, emb, scale, dout)
    torch.cuda.synchronize()
    for t in (out, lse, dqk, dv):
        assert torch.isfinite(t).all()
    assert float(lse.abs().max()) > 40                         # the logits really are large
    slack = 0.01 * float(a.abs().max())
    lo, hi = a.amin(dim=-1, keepdim=True) - slack, a.amax(dim=-1, keepdim=True) + slack
    assert bool(((out >= lo) & (out <= hi)).all())


def test_attention_bf16_bit_identical_across_runs_and_streams():
    qk, a, qb, bucket, emb = make(2, 448, 64, True)
    dout = ac.make_dout(a.shape, seed=9).cuda()
    r1 = run(qk, a, qb, bucket, emb, 448 ** -0.5, dout)
    r2 = run(qk, a, qb, bucket, emb, 448 ** -0.5, dout)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        r3 = run(qk, a, qb, bucket, emb, 448 ** -0.5, dout)
    side.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(r1, r2))
    assert all(torch.equal(x, y) for x, y in zip(r1, r3))


def test_attention_bf16_refusals():
    """F = 96, NULL and misaligned pointers, a bucket table without its embedding: BABE_ERR_ARG before any launch."""
    from babe_amd import ops
    from babe_amd._lib import BabeHipError, lib
    a = torch.zeros(1, H, 96, 16, device="cuda")
    qk = torch.zeros(1, 2 * H * 96, 16, device="cuda")
    lse = torch.empty(1, H, 16, device="cuda")
    with pytest.raises(BabeHipError):
        ops.attn_fwd(qk, a, torch.empty_like(a), lse, 0.1, precision="bf16")
    with pytest.raises(BabeHipError):
        ops.attn_vjp(qk, a, torch.empty_like(a), lse, torch.empty_like(a), torch.empty_like(qk), torch.empty_like(a), 0.1,
                     precision="bf16")
    L = lib()
    a = torch.zeros(1, H, 64, 16, device="cuda")
    qk = torch.zeros(1, 2 * H * 64, 16, device="cuda")
    o, dqk, dv, D = torch.empty_like(a), torch.empty_like(qk), torch.empty_like(a), torch.empty_like(lse)
    P = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    fwd = lambda *ptrs: L.babe_attn_fwd_bf16(*ptrs[:5], 0, *ptrs[5:], 1, H, 64, 16, 0.125, None)
    vjp = lambda *ptrs: L.babe_attn_vjp_bf16(*ptrs[:5], 0, *ptrs[5:], 1, H, 64, 16, 0.125, None)
    good_f = [P(qk), None, P(a), None, None, P(o), P(lse)]
    good_v = [P(qk), None, P(a), None, None, P(o), P(lse), P(a), P(D), P(dqk), P(dv)]
    for i in (0, 2, 5, 6):                                     # NULL qk, a, out, lse
        bad = list(good_f)
        bad[i] = None
        assert fwd(*bad) == -1 and b"null" in L.babe_last_error()
    for i in (0, 2, 5, 6, 7, 8, 9, 10):
        bad = list(good_v)
        bad[i] = None
        assert vjp(*bad) == -1 and b"null" in L.babe_last_error()
    for i, t in ((0, qk), (2, a), (5, o), (6, lse)):           # a float pointer two bytes off
        bad = list(good_f)
        bad[i] = P(t, 2)
        assert fwd(*bad) == -1 and b"aligned" in L.babe_last_error()
    bad = list(good_v)
    bad[9] = P(dqk, 2)
    assert vjp(*bad) == -1 and b"aligned" in L.babe_last_error()
    bad = list(good_f)
    bad[3] = P(torch.zeros(31, dtype=torch.int32, device="cuda"))
    assert fwd(*bad) == -1 and b"go together" in L.babe_last_error()
    torch.cuda.synchronize()
