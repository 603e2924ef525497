"""Shapes, bars and float64 models of training on the bf16 attention core: the relative-position table gradient
(babe_attn_param_vjp_bf16, csrc/attention_bf16.hip) and the qk weight gradient on bf16 MFMA (babe_attn_qk_wgrad_bf16,
csrc/attention_train.hip), shared by test_attention_bf16_train_cpu.py, test_gpu_attention_bf16_grads.py and
test_gpu_unet_attention_bf16_train.py.

Table gradient.  demb[b][k][h] = scale * sum_{n,m : bucket[m - n + T - 1] = k} dS[b,h,n,m], dS = P o (dP - D), under the rounding
model of tests/attention_bf16_cases.py: Q + bias, K + bias, V and dO rounded once to bf16, everything else exact; what is summed
is the fp32 (here: float64) dS, BEFORE it is rounded for the second product.  `rounded=False` is the exact float64 result on the
unrounded inputs.  Errors are per batch row (the outputs are per row; one wrong row must not hide in a norm over the batch).

Bars.
  BAR_DEMB = 7e-3              kernel against the exact model, per row.  The rounded model against the exact one gives
                               2.2e-3 ... 3.3e-3 per row over CPU_SHAPES (half the bar, asserted by the CPU test): the bar is 2x
                               the model, the margin the forward, dqk and dv bars carry.
  BAR_DQK_T1 (1e-2, absolute)  at T = 1 the exact demb is zero (one key: P = 1, dS = 0).
  BAR_DEMB_VS_MODEL            kernel against the ROUNDED model, per row; 2x the worst value measured on a MI355X over
  BAR_DEMB_VS_MODEL_OUT        GPU_SHAPES x B in {1, 2} x bias on / off: the model as it stands, and the model with D taken from
                               the forward's own output, where what is left is the fp32 accumulation of the scores, of D and
                               of the diagonal sums, and expf (see MEASURED_DEMB_VS_MODEL below for why there are two).
  BAR_QK_MODEL = (5e-4, 1e-2)  whole-tensor error of the float64 product of bf16-rounded operands against the unrounded one
                               (2.3e-3 ... 2.4e-3 for Gaussian operands): below the window the bf16 pipe did not run, above it
                               something other than one rounding per operand happened.
  TOL_FP32_ACC = 2e-5          fp32 accumulation against float64 of the same (rounded) operands: the bar of
                               tests/test_gpu_wgrad_bf16.py, and of the qk-bias row sum.

Network (test_gpu_unet_attention_bf16_train.py): parameter gradients of an f32 network with the bf16 core under
set_trainable(True, attention='bf16') against the same network on the fp32 core (attention=True, which
tests/test_gpu_unet_attention_train.py pins to the reference at 2e-4).  NET_BAR_KEY / NET_BAR_WHOLE are 2x the worst per-key /
whole-gradient relative error measured over fixtures "a" and "b" (MEASURED_NET); a per-key value above NET_FINDING = 7.5e-3 (half
the project's per-product bf16 bar of 1.5e-2) would be a finding to explain, not a bar to widen."""
import torch

from tests.attention_bf16_cases import BAR_DQK_T1, H, make_cpu, make_dout  # noqa: F401  (re-exported)

CPU_SHAPES = [(64, 8), (64, 17), (64, 33), (64, 37), (64, 129), (128, 100), (320, 100), (448, 64), (64, 1024)]
# the waves of the table pass: T = 1, 8, 15, 16 leave the st = 1 waves and the rt = 1 pair idle; 17 gives each one row; 31, 32,
# 33 sit around one full workgroup / chunk; 129 has more chunks than waves; 1024 is the long-T level; (320, 100), (448, 64): the
# wide heads (LDS images of 114 KiB at F = 448), ragged T
GPU_SHAPES = [(64, 1), (64, 8), (64, 15), (64, 16), (64, 17), (64, 31), (64, 32), (64, 33), (64, 129), (64, 1024), (320, 100),
              (448, 64)]
QK_SHAPES = [(64, 1, 1), (64, 8, 3), (64, 37, 2), (64, 129, 2), (64, 1024, 3), (448, 64, 2), (320, 100, 1)]     # (F, T, B)
QK_MODEL_SHAPES = [(64, 1, 1), (64, 8, 3), (64, 37, 2), (64, 129, 2)]

BAR_DEMB = 7e-3
BAR_QK_MODEL = (5e-4, 1e-2)
TOL_FP32_ACC = 2e-5

# Kernel against the rounded model, worst batch row, measured on a MI355X: {(F, T): worst over B in {1, 2} and bias on / off}.
# Up to T = 16 the kernel sits on the model (2e-7); from T = 17 on it does not, and at T = 1024 the value passes the 1e-3 above
# which the kernel is the first suspect.  The cause is D = sum_f dO O, not the table pass: the model forms D from ITS forward
# output, which rounds exp(S - max) against the row's final maximum, while babe_attn_fwd_bf16 rounds against the running maximum
# of each wave's half of the keys (the online rescaling the model of tests/attention_bf16_cases.py leaves out) - a different
# bf16 rounding of the same probabilities as soon as a row has more than one key tile (T >= 17), and D multiplies every dS of
# the row.  With D formed from the forward's own output and everything else as in the model (demb_model(out=)), what is left is
# fp32 accumulation: MEASURED_DEMB_VS_MODEL_OUT, 1.3e-6 at the worst.  Both bars are 2x the worst measurement.
MEASURED_DEMB_VS_MODEL = {(64, 8): 1.97e-7, (64, 15): 1.70e-5, (64, 16): 2.12e-7, (64, 17): 2.07e-4, (64, 31): 5.40e-4,
                          (64, 32): 5.25e-4, (64, 33): 5.97e-4, (64, 129): 1.01e-3, (64, 1024): 3.29e-3, (320, 100): 6.68e-4,
                          (448, 64): 5.85e-4}
MEASURED_DEMB_VS_MODEL_OUT = {(64, 8): 1.93e-7, (64, 15): 2.16e-7, (64, 16): 2.08e-7, (64, 17): 2.15e-7, (64, 31): 2.92e-7,
                              (64, 32): 2.87e-7, (64, 33): 2.82e-7, (64, 129): 4.59e-7, (64, 1024): 1.32e-6, (320, 100): 4.06e-7,
                              (448, 64): 4.06e-7}
BAR_DEMB_VS_MODEL = 2 * max(MEASURED_DEMB_VS_MODEL.values())                # 6.6e-3
BAR_DEMB_VS_MODEL_OUT = 2 * max(MEASURED_DEMB_VS_MODEL_OUT.values())        # 2.6e-6

# bf16 core (attention='bf16') against the fp32 core (attention=True), f32 network, measured on a MI355X:
# {fixture: (worst key, its relative error, whole-gradient relative error)}.  Both bars are 2x the worst measurement.
MEASURED_NET = {"a": ("ups.2.1.attn_block.qk.weight", 3.856e-3, 1.094e-4),
                "b": ("ups.6.1.attn_block.qk.bias", 2.267e-2, 6.490e-4)}
NET_BAR_KEY = 2 * max(v[1] for v in MEASURED_NET.values())         # 4.5e-2
NET_BAR_WHOLE = 2 * max(v[2] for v in MEASURED_NET.values())       # 1.3e-3
# The finding above NET_FINDING.  In fixture "a" every key is below 3.9e-3.  In fixture "b" (attention at all eight levels, qk
# bias, no table) every key is below 6e-3 except gradients of the qk Conv1d in the up path: qk.bias of ups.2.1 / 3.1 / 4.1 / 6.1
# (1.14e-2, 9.1e-3, 7.8e-3, 2.27e-2) and qk.weight of ups.6.1 (1.27e-2).  All of them are fp32 linear maps (the fixed-order row
# sum; babe_attn_qk_wgrad) of the dqk that babe_attn_vjp_bf16 writes - no kernel of the training path that is new with the bf16
# opt-in is involved (wgrad is None in this test).  What is measured: the key half of the bias gradient is zero mathematically
# (a constant added to every key moves no softmax) - the fp32 core leaves 6e-7 |g| there, the bf16 core 1.8e-2 |g| at ups.6.1,
# 2e-3 ... 9e-3 |g| elsewhere.  The core rounds each dS to bf16 for the dS K and dS^T Q products, so sum_m dS[n, m] = 0 holds to
# 2^-9 per term only, and whatever cancels through that identity (the key bias entirely; the time-constant part of K in the
# query rows, of a1 in the weight gradient) leaves its rounding noise behind while its signal is gone.  That the query rows
# (1.3e-2) and the weight gradient of ups.6.1 follow the same mechanism is an inference from that measurement, not a measurement;
# both stay inside the 1.5e-2 per-column bar the bf16 core's dqk is held to (tests/attention_bf16_cases.py).
NET_FINDING = 7.5e-3
NET_FINDING_KEYS = ("attn_block.qk.bias", "attn_block.qk.weight")   # linear in the bf16 core's dqk: held to NET_BAR_KEY only


def _bf(x):
    return x.float().bfloat16().double()


def demb_model(qk, a, qb, bucket, emb, scale, dout, rounded, out=None):
    """demb [B, nb, H] in float64 on the tensors' device: the rounding model of the module docstring, or the exact result.
    out: the forward's output that D = sum_f dO O is formed from (None: the model's own)."""
    B, Hh, F, T = a.shape
    r = _bf if rounded else (lambda x: x.double())
    x = qk.float() if qb is None else qk.float() + qb.float()[None, :, None]           # fp32, as the kernels add it
    x = x.reshape(B, Hh, 2, F, T)
    q, k, v, do = r(x[:, :, 0]), r(x[:, :, 1]), r(a), r(dout)
    idx = torch.arange(T, device=a.device)[None, :] - torch.arange(T, device=a.device)[:, None] + T - 1          # [n][m]
    bk = bucket.long()[idx]                                                             # [n][m] -> bucket
    s = torch.einsum("bhfn,bhfm->bhnm", q, k) + emb.double()[bk].permute(2, 0, 1)[None]
    s = s * scale
    e = (s - s.amax(dim=-1, keepdim=True)).exp()
    den = e.sum(dim=-1, keepdim=True)
    p = e / den
    if out is None:
        out = torch.einsum("bhnm,bhfm->bhfn", r(e), v) / den.transpose(-1, -2)          # the forward's output, as the model has it
    D = (dout.double() * out.double()).sum(2)                                           # dO unrounded
    dp = torch.einsum("bhfn,bhfm->bhnm", do, v)
    ds = p * (dp - D[..., None])                                                        # summed unrounded
    nb = emb.shape[0]
    demb = torch.zeros(B, Hh, nb, device=a.device, dtype=torch.float64)
    demb.index_add_(2, bk.reshape(-1), ds.reshape(B, Hh, T * T))
    return scale * demb.transpose(1, 2).contiguous()


def rel_rows(x, ref):
    """Worst relative error over the batch rows x[b] (2-norm over everything else)."""
    x, ref = x.detach().double().cpu(), ref.detach().double().cpu()
    B = x.shape[0]
    num = (x - ref).reshape(B, -1).norm(dim=1)
    den = ref.reshape(B, -1).norm(dim=1)
    return float((num / (den + 1e-300)).max())


def qk_operands(F, T, B, device="cpu"):
    """dqk [B, 2HF, T] and a1 [B, HF, T] of tests/test_gpu_attention_grads.py::test_attn_qk_wgrad_vs_float64 (same generator)."""
    HF = H * F
    g = torch.Generator().manual_seed(17 * F + T)
    dqk = torch.randn(B, 2 * HF, T, generator=g)
    a1 = torch.randn(B, HF, T, generator=g)
    return dqk.to(device), a1.to(device)


def qk_product(dqk, a1, rounded):
    """sum_b dqk[b] a1[b]^T in float64, of the bf16-rounded or of the unrounded operands."""
    r = _bf if rounded else (lambda x: x.double())
    return torch.einsum("bot,bit->oi", r(dqk), r(a1))


TIE_LO, TIE_HI = 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8       # both halfway between two bf16 values: to even -> 1 and 1 + 2^-6


def qk_tie_inputs(HF=512, T=24, B=2):
    """a1 alternates the two tie values (in a pattern that differs from row to row); dqk holds a single 1.0 per output row (in
    batch row co % B), so every entry of dW is one rounded a1 value: exact in any arithmetic, and 1 or 1 + 2^-6 only if the
    rounding is to nearest even (truncation gives 1 and 1 + 2^-7, round-half-up 1 + 2^-7 and 1 + 2^-6)."""
    i = torch.arange(B * HF * T).reshape(B, HF, T)
    a1 = torch.where((i * 7 // 3 + i // T) % 2 == 0, torch.tensor(TIE_LO), torch.tensor(TIE_HI)).float()
    assert set(a1.unique().tolist()) == {TIE_LO, TIE_HI}
    dqk = torch.zeros(B, 2 * HF, T)
    for co in range(2 * HF):
        dqk[co % B, co, (co * 11) % T] = 1.0
    return dqk, a1
