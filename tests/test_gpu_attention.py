"""Time-attention kernels (csrc/attention.hip) against a float64 torch restatement of the reference's TimeAttentionBlock core:
forward and input-VJP at the UNet's head shapes, ragged T, B = 1 and 2, relative bias on and off.  Needs a MI355X."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(64, 8), (448, 64), (320, 100), (320, 256), (64, 1024), (64, 4096)]
H = 8


def ref_attn(qk, a, scale, qk_bias=None, bucket=None, emb=None):
    """float64: qk [B,2HF,T], a [B,H,F,T] -> out [B,H,F,T] (reference: einops 'b (h d) t -> b h t d', chunk, einsum)."""
    B, Hh, F, T = a.shape
    if qk_bias is not None:
        qk = qk + qk_bias[None, :, None]
    qk = qk.reshape(B, Hh, 2 * F, T).transpose(-1, -2)          # b h t d
    q, k = qk.chunk(2, dim=-1)
    v = a.transpose(-1, -2)
    sim = torch.einsum("bhnd,bhmd->bhnm", q, k)
    if bucket is not None:
        idx = torch.arange(T, device=a.device)[None, :] - torch.arange(T, device=a.device)[:, None] + T - 1
        sim = sim + emb[bucket.long()[idx]].permute(2, 0, 1)[None]
    attn = (sim * scale).softmax(dim=-1)
    return torch.einsum("bhnm,bhmd->bhnd", attn, v).transpose(-1, -2)


def rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-300))


def make(B, F, T, rel_pos, bias=False, amp=1.0, seed=0):
    from babe_amd import ops
    g = torch.Generator().manual_seed(seed + 1000 * F + T)
    qk = (amp * torch.randn(B, 2 * H * F, T, generator=g) / F ** 0.25).cuda()
    a = torch.randn(B, H, F, T, generator=g).cuda()
    qb = (0.1 * torch.randn(2 * H * F, generator=g)).cuda() if bias else None
    bucket = ops.attn_buckets(T).cuda() if rel_pos else None
    emb = torch.randn(32, H, generator=g).cuda() if rel_pos else None
    return qk, a, qb, bucket, emb


def run(qk, a, qb, bucket, emb, scale, dout=None):
    from babe_amd import ops
    B, Hh, F, T = a.shape
    out = torch.empty_like(a)
    lse = torch.empty(B, Hh, T, device=a.device)
    ops.attn_fwd(qk, a, out, lse, scale, qk_bias=qb, bucket=bucket, emb=emb)
    if dout is None:
        return out, lse
    dqk, dv = torch.empty_like(qk), torch.empty_like(a)
    ops.attn_vjp(qk, a, out, lse, dout, dqk, dv, scale, qk_bias=qb, bucket=bucket, emb=emb)
    return out, lse, dqk, dv


def ref_grads(qk, a, qb, bucket, emb, scale, dout):
    q64, a64 = qk.double().requires_grad_(True), a.double().requires_grad_(True)
    o = ref_attn(q64, a64, scale, None if qb is None else qb.double(), bucket, None if emb is None else emb.double())
    gq, ga = torch.autograd.grad((o * dout.double()).sum(), (q64, a64))
    return o.detach(), gq, ga


@pytest.mark.parametrize("F,T", SHAPES)
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("rel_pos", [True, False])
def test_attention_fwd_vjp_vs_float64(F, T, B, rel_pos):
    qk, a, qb, bucket, emb = make(B, F, T, rel_pos, bias=not rel_pos)
    scale = F ** -0.5
    dout = torch.randn(a.shape, generator=torch.Generator().manual_seed(7)).cuda()
    out, lse, dqk, dv = run(qk, a, qb, bucket, emb, scale, dout)
    torch.cuda.synchronize()
    o64, gq, ga = ref_grads(qk, a, qb, bucket, emb, scale, dout)
    eo, eq = rel(out, o64), rel(dqk, gq)
    ev = rel(dv, ga)                               # dv is the V part of the gradient w.r.t. a (qk's own path is the conv's)
    print(f"F={F} T={T} B={B} rel_pos={rel_pos}: fwd {eo:.2e} dqk {eq:.2e} dv {ev:.2e}")
    assert eo <= 2e-5 and eq <= 2e-5 and ev <= 2e-5


def test_attention_large_logits_stay_finite():
    """Scores scaled to about +-80: the online softmax must not overflow (no inf / NaN) and still match float64."""
    F, T = 320, 100
    qk, a, qb, bucket, emb = make(1, F, T, True, amp=1.0)
    scale = F ** -0.5
    # scale q so that max |S| ~ 80
    qk = qk.view(1, H, 2, F, T)
    q, k = qk[:, :, 0].double(), qk[:, :, 1].double()
    smax = float(torch.einsum("bhfn,bhfm->bhnm", q, k).abs().max()) * scale
    qk[:, :, 0] *= 80.0 / smax
    qk = qk.reshape(1, 2 * H * F, T).contiguous()
    dout = torch.randn(a.shape, generator=torch.Generator().manual_seed(3)).cuda()
    out, lse, dqk, dv = run(qk, a, qb, bucket, emb, scale, dout)
    torch.cuda.synchronize()
    for t in (out, lse, dqk, dv):
        assert torch.isfinite(t).all()
    o64, gq, ga = ref_grads(qk, a, qb, bucket, emb, scale, dout)
    # (fp32 rounding of a score of 80 is ~5e-6 absolute, amplified in the sharp softmax: looser bars than the O(1) shapes)
    assert rel(out, o64) <= 1e-4 and rel(dv, ga) <= 1e-3 and rel(dqk, gq) <= 1e-3


def test_attention_two_runs_bit_identical():
    qk, a, qb, bucket, emb = make(2, 448, 64, True)
    dout = torch.randn(a.shape, generator=torch.Generator().manual_seed(9)).cuda()
    r1 = run(qk, a, qb, bucket, emb, 448 ** -0.5, dout)
    r2 = run(qk, a, qb, bucket, emb, 448 ** -0.5, dout)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(r1, r2))


def test_attention_rejects_unsupported_head_dim():
    from babe_amd import ops
    from babe_amd._lib import BabeHipError
    a = torch.zeros(1, H, 96, 16, device="cuda")
    qk = torch.zeros(1, 2 * H * 96, 16, device="cuda")
    with pytest.raises(BabeHipError):
        ops.attn_fwd(qk, a, torch.empty_like(a), torch.empty(1, H, 16, device="cuda"), 0.1)
