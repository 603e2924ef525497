"""Shapes, bars and float64 models of the bf16 time-attention kernels (babe_attn_fwd_bf16 / babe_attn_vjp_bf16,
csrc/attention_bf16.hip), shared by the CPU model test (test_attention_bf16_cpu.py) and the GPU test (test_gpu_attention_bf16.py).

Rounding model (`model(..., rounded=True)`), in float64 apart from the roundings themselves:
  * Q + bias and K + bias (the bias added in fp32 first), V and dO are rounded once to bf16, to nearest even;
  * S, the softmax maximum / sum and the probabilities P are exact; the denominator sums the unrounded exponentials;
  * P is rounded to bf16 for P V and P^T dO only, dS = P o (dP - D) for dS K and dS^T Q only (dS is formed from the unrounded P);
    the forward rounds the unnormalised exp(S - max) and divides the product by the denominator afterwards, as the kernel does
    (the row's largest probability is then exact), the VJP rounds P = exp(S - lse);
  * D = sum_f dO O uses the unrounded dO and the model's own output.
`rounded=False` is the exact float64 result on the unrounded inputs, the reference of both tests.  What the model leaves out is
the fp32 accumulation order and the online rescaling of the kernels; the bars carry about 2x over the model for those.

Bars (whole tensor: |x - ref| / |ref| in the 2-norm; per time column: the same over every time column
x[b, ..., n] of a batch item separately, so that one wrong row cannot hide in a norm; 1.5e-2 is the project's per-product bf16 bar).  At T = 1 the exact dqk is zero (one key:
P = 1, dS = 0) and its bar is absolute."""
import torch

H = 8
# (F, T) pairs of the CPU model test ...
CPU_SHAPES = [(64, 1), (64, 15), (64, 16), (64, 17), (64, 33), (128, 100), (448, 64), (320, 256)]
# ... and of the GPU test.  The kernels give a workgroup of four waves 32 own rows (wave pair rt = 0, 1: 16 rows each) and walk
# the other side in chunks of 32 (wave st = 0, 1 of a pair: 16 streamed rows each):
#   T = 1, 15, 16   the st = 1 waves get no key / query at all and the rt = 1 pair owns no row: the (-inf, 0, 0) partials
#   T = 17          the st = 1 wave gets exactly one streamed row, the rt = 1 pair one own row
#   T = 31, 32, 33  one short of filling every part of one workgroup and one chunk, exactly full, one past (a second workgroup
#                   with one own row, a second chunk with one streamed row)
#   T = 65, 129     more chunks than waves; T = 1024: 32 workgroups x 32 chunks, the long-T layers
#   (448, 64), (448, 1): the largest head (LDS images of 150 KiB, 112 accumulator registers), (320, 100), (128, 257): ragged T
GPU_SHAPES = [(64, 1), (64, 15), (64, 16), (64, 17), (64, 31), (64, 32), (64, 33), (64, 65), (64, 129), (64, 1024),
              (448, 64), (448, 1), (320, 100), (128, 257)]

BAR = {"out": 5e-3, "dqk": 7e-3, "dv": 5e-3}     # whole tensor
BAR_COLUMN = 1.5e-2                              # every time column separately
BAR_DQK_T1 = 1e-2                                # max |dqk| at T = 1


def make_cpu(B, F, T, rel_pos, bias=False, amp=1.0, seed=0):
    """The CPU tensors of tests/test_gpu_attention.py::make (same generator, same order): qk, a, qb, bucket, emb."""
    from babe_amd import ops
    g = torch.Generator().manual_seed(seed + 1000 * F + T)
    qk = amp * torch.randn(B, 2 * H * F, T, generator=g) / F ** 0.25
    a = torch.randn(B, H, F, T, generator=g)
    qb = 0.1 * torch.randn(2 * H * F, generator=g) if bias else None
    bucket = ops.attn_buckets(T) if rel_pos else None
    emb = torch.randn(32, H, generator=g) if rel_pos else None
    return qk, a, qb, bucket, emb


def make_dout(shape, seed=7):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _bf(x):
    return x.float().bfloat16().double()


def model(qk, a, qb, bucket, emb, scale, dout, rounded):
    """(out, dqk, dv) in float64 on the tensors' device: the rounding model of the module docstring, or the exact result."""
    B, Hh, F, T = a.shape
    r = _bf if rounded else (lambda x: x.double())
    x = qk.float() if qb is None else qk.float() + qb.float()[None, :, None]           # fp32, as the kernels add it
    x = x.reshape(B, Hh, 2, F, T)
    q, k, v, do = r(x[:, :, 0]), r(x[:, :, 1]), r(a), r(dout)
    s = torch.einsum("bhfn,bhfm->bhnm", q, k)
    if bucket is not None:
        idx = torch.arange(T, device=a.device)[None, :] - torch.arange(T, device=a.device)[:, None] + T - 1      # [n][m]: m - n + T - 1
        s = s + emb.double()[bucket.long()[idx]].permute(2, 0, 1)[None]
    s = s * scale
    e = (s - s.amax(dim=-1, keepdim=True)).exp()
    den = e.sum(dim=-1, keepdim=True)                                                   # the unrounded exponentials
    p = e / den
    out = torch.einsum("bhnm,bhfm->bhfn", r(e), v) / den.transpose(-1, -2)              # forward: exp(S - max) is what is rounded
    pr = r(p)                                                                           # VJP: P = exp(S - lse)
    D = (dout.double() * out).sum(2)                                                    # [B,H,T], dO unrounded
    dp = torch.einsum("bhfn,bhfm->bhnm", do, v)
    ds = p * (dp - D[..., None])
    dsr = r(ds)
    dq = scale * torch.einsum("bhnm,bhfm->bhfn", dsr, k)
    dk = scale * torch.einsum("bhnm,bhfn->bhfm", dsr, q)
    dv = torch.einsum("bhnm,bhfn->bhfm", pr, do)
    dqk = torch.stack([dq, dk], 2).reshape(B, 2 * Hh * F, T)
    return out, dqk, dv


def rel(x, ref):
    x, ref = x.detach().double().cpu(), ref.detach().double().cpu()
    return float((x - ref).norm() / (ref.norm() + 1e-300))


def rel_columns(x, ref):
    """Worst relative error over the time columns x[b, ..., n] of out / dv [B,H,F,T] and dqk [B,2HF,T]: the norm runs over every
    row of one batch item at one time step."""
    x, ref = x.detach().double().cpu(), ref.detach().double().cpu()
    B, T = x.shape[0], x.shape[-1]
    num = (x - ref).reshape(B, -1, T).norm(dim=1)
    den = ref.reshape(B, -1, T).norm(dim=1)
    return float((num / (den + 1e-300)).max())


def errors(got, ref):
    """{name: (whole-tensor error, worst column error)} of (out, dqk, dv) tuples; dqk at T = 1: (max |dqk|, None)."""
    res = {}
    for name, x, r_ in zip(("out", "dqk", "dv"), got, ref):
        if name == "dqk" and x.shape[-1] == 1:
            res[name] = (float(x.detach().abs().max()), None)
        else:
            res[name] = (rel(x, r_), rel_columns(x, r_))
    return res


def check(errs, frac=1.0):
    """Assert `errs` (from errors) within frac x the bars."""
    for name, (whole, col) in errs.items():
        if col is None:
            assert whole <= frac * BAR_DQK_T1, (name, whole)
        else:
            assert whole <= frac * BAR[name], (name, whole)
            assert col <= frac * BAR_COLUMN, (name, "column", col)
