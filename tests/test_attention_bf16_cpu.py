"""The float64 rounding model of the bf16 attention kernels (tests/attention_bf16_cases.py) against the exact float64 result:
the model's error is at most half of every bar the GPU test applies, and it is not zero - the bars are neither vacuous nor tight.
No GPU."""
import pytest
import torch

from tests import attention_bf16_cases as ac


def _exact_by_autograd(qk, a, qb, bucket, emb, scale, dout):
    """The exact result once more, by autograd through the plain softmax attention: pins model(rounded=False) itself."""
    B, Hh, F, T = a.shape
    q64, a64 = qk.double().requires_grad_(True), a.double().requires_grad_(True)
    x = q64 if qb is None else q64 + qb.double()[None, :, None]
    x = x.reshape(B, Hh, 2, F, T)
    s = torch.einsum("bhfn,bhfm->bhnm", x[:, :, 0], x[:, :, 1])
    if bucket is not None:
        idx = torch.arange(T)[None, :] - torch.arange(T)[:, None] + T - 1
        s = s + emb.double()[bucket.long()[idx]].permute(2, 0, 1)[None]
    o = torch.einsum("bhnm,bhfm->bhfn", (s * scale).softmax(-1), a64)
    gq, ga = torch.autograd.grad((o * dout.double()).sum(), (q64, a64))
    return o.detach(), gq, ga


@pytest.mark.parametrize("F,T", ac.CPU_SHAPES)
@pytest.mark.parametrize("rel_pos", [True, False])
def test_rounding_model_within_half_of_every_bar(F, T, rel_pos):
    qk, a, qb, bucket, emb = ac.make_cpu(2, F, T, rel_pos, bias=not rel_pos)
    scale = F ** -0.5
    dout = ac.make_dout(a.shape)
    exact = ac.model(qk, a, qb, bucket, emb, scale, dout, rounded=False)
    errs = ac.errors(ac.model(qk, a, qb, bucket, emb, scale, dout, rounded=True), exact)
    print(f"F={F} T={T} rel_pos={rel_pos}: " + ", ".join(f"{k} {w:.2e}" + (f" (column {c:.2e})" if c is not None else "")
                                                         for k, (w, c) in errs.items()))
    ac.check(errs, frac=0.5)
    for name, (whole, col) in errs.items():              # the rounding is visible: a bar of this size is not vacuous
        assert whole >= (1e-4 if col is None else 1e-3), (name, whole)


def test_exact_model_is_the_softmax_attention():
    for rel_pos in (True, False):
        qk, a, qb, bucket, emb = ac.make_cpu(2, 64, 33, rel_pos, bias=not rel_pos)
        dout = ac.make_dout(a.shape)
        got = ac.model(qk, a, qb, bucket, emb, 0.125, dout, rounded=False)
        ref = _exact_by_autograd(qk, a, qb, bucket, emb, 0.125, dout)
        for g_, r_ in zip(got, ref):
            # (the model adds the qk bias in fp32, as the kernels do: 1e-7 of the float64 sum)
            assert ac.rel(g_, r_) < 1e-6
