"""Parameter-gradient kernels of the time-attention branch (csrc/attention_train.hip) against float64 autograd of a torch
restatement, H = 8: the relative-position table and qk-bias gradients (attn_param_vjp), the batch-summed qk weight gradient
(attn_qk_wgrad) and GroupNorm * FiLM without GELU (gn_param_grad_nogelu).  The 2e-5 bar is the one tests/test_gpu_attention.py
holds the attention VJP to.  Needs a MI355X."""
import pytest
import torch

from tests.test_gpu_attention import H, make, ref_attn, rel, run

pytestmark = pytest.mark.gpu
TOL = 2e-5


def nan_rows(B, n, pad=3):
    """A [B, n] view with a row stride larger than n inside a NaN-filled buffer (the layout of ParamGrads.rows)."""
    buf = torch.full((B, n + 2 * pad), float("nan"), device="cuda")
    return buf, buf[:, pad:pad + n]


@pytest.mark.parametrize("F,T", [(64, 8), (64, 37), (320, 100), (448, 64), (64, 1024)])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("bias", [False, True])
def test_attn_param_vjp_vs_float64(F, T, B, bias):
    """T = 100 and 1024 exceed max_distance = 64 (saturated end buckets), T = 37 and 100 have ragged last tiles, T = 8 leaves
    buckets that no (query, key) pair reaches: those must come out as exactly 0.0 over the NaN pre-fill."""
    from babe_amd import ops
    qk, a, qb, bucket, emb = make(B, F, T, True, bias=bias)
    scale = F ** -0.5
    dout = torch.randn(a.shape, generator=torch.Generator().manual_seed(11)).cuda()
    out, lse, dqk, dv = run(qk, a, qb, bucket, emb, scale, dout)
    ebuf, demb = nan_rows(B, 32 * H)
    bbuf, dqkb = nan_rows(B, 2 * H * F)
    ops.attn_param_vjp(qk, a, out, lse, dout, dqk, scale, qk_bias=qb, bucket=bucket, emb=emb, demb_rows=demb, dqkb_rows=dqkb)
    torch.cuda.synchronize()
    assert torch.isnan(ebuf[:, :3]).all() and torch.isnan(ebuf[:, -3:]).all() and torch.isnan(bbuf[:, :3]).all()
    # float64 autograd, one batch row at a time (the outputs are per row); a zero bias stands in where the case has none
    want_e, want_b = [], []
    for b in range(B):
        e64 = emb.double().requires_grad_(True)
        b64 = (qb.double() if bias else torch.zeros(2 * H * F, device="cuda", dtype=torch.float64)).requires_grad_(True)
        o = ref_attn(qk[b:b + 1].double(), a[b:b + 1].double(), scale, b64, bucket, e64)
        ge, gb = torch.autograd.grad((o * dout[b:b + 1].double()).sum(), (e64, b64))
        want_e.append(ge.reshape(-1))
        want_b.append(gb)
    want_e, want_b = torch.stack(want_e), torch.stack(want_b)
    ee, eb = rel(demb, want_e), rel(dqkb, want_b)
    print(f"F={F} T={T} B={B} bias={bias}: demb {ee:.2e} dqkb {eb:.2e}")
    assert torch.isfinite(demb).all() and torch.isfinite(dqkb).all()
    assert ee <= TOL and eb <= TOL
    reached = torch.zeros(32, dtype=torch.bool)
    reached[bucket.cpu().long()] = True
    if T == 8:
        assert not reached.all()
    assert (demb.view(B, 32, H)[:, ~reached] == 0.0).all()


@pytest.mark.parametrize("F,T", [(64, 33), (448, 64)])
def test_attn_param_vjp_is_deterministic_and_row_independent(F, T):
    """Two runs bit for bit, and row 1 of a B = 2 call equals the B = 1 call on that row: the kernels' header promises fixed
    summation orders and per-row outputs that do not depend on which other rows share the call (a training step may split its
    batch rows between calls).  T = 33 has three key tiles with a ragged last one, F = 448 is the widest head."""
    from babe_amd import ops

    def grads(qk, a, dout):
        out, lse, dqk, _ = run(qk, a, qb, bucket, emb, scale, dout)
        demb = torch.full((qk.shape[0], 32 * H), float("nan"), device="cuda")
        dqkb = torch.full((qk.shape[0], 2 * H * F), float("nan"), device="cuda")
        ops.attn_param_vjp(qk, a, out, lse, dout, dqk, scale, qk_bias=qb, bucket=bucket, emb=emb, demb_rows=demb, dqkb_rows=dqkb)
        torch.cuda.synchronize()
        return demb, dqkb

    qk, a, qb, bucket, emb = make(2, F, T, True, bias=True)
    scale = F ** -0.5
    dout = torch.randn(a.shape, generator=torch.Generator().manual_seed(11)).cuda()
    demb, dqkb = grads(qk, a, dout)
    demb2, dqkb2 = grads(qk, a, dout)
    assert torch.isfinite(demb).all() and torch.isfinite(dqkb).all()
    assert torch.equal(demb, demb2) and torch.equal(dqkb, dqkb2)
    demb1, dqkb1 = grads(qk[1:].contiguous(), a[1:].contiguous(), dout[1:].contiguous())
    assert torch.equal(demb[1:], demb1) and torch.equal(dqkb[1:], dqkb1)


@pytest.mark.parametrize("F,T,B", [(64, 1, 1), (64, 8, 3), (64, 37, 2), (64, 1024, 3), (448, 64, 2), (320, 100, 1)])
def test_attn_qk_wgrad_vs_float64(F, T, B):
    """T = 1, T not a multiple of 4 (rows not 16-byte aligned), the K-split levels (F = 64) and the single-chunk ones, beta = 0
    over a NaN-filled output, beta = 1 accumulation, and two runs bit for bit."""
    from babe_amd import ops
    HF = H * F
    g = torch.Generator().manual_seed(17 * F + T)
    dqk = torch.randn(B, 2 * HF, T, generator=g).cuda()
    a1 = torch.randn(B, HF, T, generator=g).cuda()
    want = torch.zeros(2 * HF, HF, device="cuda", dtype=torch.float64)
    for b in range(B):
        want += dqk[b].double() @ a1[b].double().t()
    dW = torch.full((2 * HF, HF), float("nan"), device="cuda")
    ops.attn_qk_wgrad(dqk, a1, dW)
    e0 = rel(dW, want)
    dW2 = torch.full((2 * HF, HF), float("nan"), device="cuda")
    ops.attn_qk_wgrad(dqk, a1, dW2)
    assert torch.equal(dW, dW2)
    del dW2
    base = torch.randn(2 * HF, HF, device="cuda")
    acc = base.clone()
    ops.attn_qk_wgrad(dqk, a1, acc, alpha=0.5, beta=1.0)
    e1 = rel(acc, base.double() + 0.5 * want)
    print(f"F={F} T={T} B={B}: beta=0 {e0:.2e}, beta=1 {e1:.2e}")
    assert e0 <= TOL and e1 <= TOL


def test_attn_qk_wgrad_refuses_shapes_outside_the_contract():
    from babe_amd import ops
    from babe_amd._lib import BabeHipError, lib, ptr
    for HF in (256, 600, 4096):
        dqk, a1 = torch.zeros(1, 2 * HF, 4, device="cuda"), torch.zeros(1, HF, 4, device="cuda")
        dW = torch.zeros(2 * HF, HF, device="cuda")
        with pytest.raises(BabeHipError):
            ops.attn_qk_wgrad(dqk, a1, dW)
        assert lib().babe_attn_qk_wgrad(ptr(dqk), ptr(a1), ptr(dW), None, 1, HF, 4, 1.0, 0.0, None) == -1
        assert b"unsupported shape" in lib().babe_last_error()
    assert lib().babe_attn_qk_wgrad(None, None, None, None, 1, 512, 4, 1.0, 0.0, None) == -1


def test_attn_param_vjp_refuses_what_does_not_fit():
    """F = 448 with T = 4096 would need more LDS than a workgroup has: an argument error, not a fault."""
    from babe_amd._lib import lib
    L = lib()
    fake = 0x10000                                            # refused before anything is dereferenced
    rc = L.babe_attn_param_vjp(fake, None, fake, fake, fake, 32, fake, fake, fake, fake, fake, fake, 256, None, 0, 1, H, 448, 4096,
                               0.05, None)
    assert rc == -1 and b"LDS" in L.babe_last_error()
    assert L.babe_attn_param_vjp(fake, None, fake, None, None, 0, fake, fake, fake, fake, fake, None, 0, None, 0, 1, H, 64, 8, 0.1,
                                 None) == -1


@pytest.mark.parametrize("shape", [(2, 16, 64, 37), (1, 8, 64, 8)])
def test_gn_param_grad_nogelu_vs_float64(shape):
    from babe_amd import ops
    B, C, F, T = shape
    G = 8
    g = torch.Generator().manual_seed(sum(shape))
    z = torch.randn(shape, generator=g).cuda()
    da = torch.randn(shape, generator=g).cuda()
    gamma = (1 + 0.2 * torch.randn(C, generator=g)).cuda()
    film = (0.3 * torch.randn(B, C + 4, generator=g)).cuda()[:, 2:2 + C]         # a column slice, as in the engine
    stats, scale = ops.gn_scale(z, gamma, film, G)
    gbuf, dg = nan_rows(B, C)
    fbuf, df = nan_rows(B, C)
    cs = 0.7
    ops.gn_param_grad_nogelu(z, da, stats, gamma, film, dg, df, cs=cs, G=G)
    torch.cuda.synchronize()
    # a = z * gamma * (film + 1) * r with r the group's 1/(std + eps) held fixed (it does not depend on gamma or film)
    r = stats[:, :, 2].double().repeat_interleave(C // G, dim=1)
    g64 = gamma.double().expand(B, C).clone().requires_grad_(True)                # one copy per row: per-row gradients
    f64 = film.double().clone().requires_grad_(True)
    a = z.double() * (g64 * (f64 + 1) * r)[:, :, None, None]
    wg, wf = torch.autograd.grad((a * (cs * da.double())).sum(), (g64, f64))
    eg, ef = rel(dg, wg), rel(df, wf)
    print(f"{shape}: dgamma {eg:.2e} dfilm {ef:.2e}")
    assert eg <= TOL and ef <= TOL
    assert rel(scale.double(), (gamma.double()[None] * (film.double() + 1) * r)) < 1e-6      # the restatement is the kernel's scale
