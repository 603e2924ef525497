"""The fused optimizer tail (csrc/optim.hip, babe_amd/optim.py) without a GPU: the host-side chunk builder, the argument checks
of the two launching entry points (made before any device call), training.ema_decay against update_ema, FusedAdamEMA's
constructor refusals and its state interchange with torch.optim.Adam."""
import ctypes as C

import numpy as np
import pytest
import torch


def _chunks(sizes, chunk, cap=None):
    from babe_amd._cabi import OptChunk
    from babe_amd._lib import lib
    L = lib()
    n = (C.c_long * len(sizes))(*sizes)
    cap = sum(-(-max(s, 0) // max(chunk, 1)) for s in sizes) + 4 if cap is None else cap
    out = (OptChunk * max(cap, 1))()
    count = L.babe_opt_chunks(n, len(sizes), chunk, out, cap)
    return count, [(out[i].t, out[i].off, out[i].n) for i in range(max(count, 0))]


def test_chunk_builder_covers_every_element_once():
    from babe_amd.optim import CHUNK as Cs
    assert Cs % 4 == 0 and Cs >= 256
    for sizes in ([1, 3, 4, 5, 63, 64, 65, 255, 256, 257, Cs - 1, Cs, Cs + 1, 2 * Cs + 7], [1]):
        count, ch = _chunks(sizes, Cs)
        assert count == sum(-(-s // Cs) for s in sizes) == len(ch)
        seen = [np.zeros(s, np.int32) for s in sizes]
        for t, off, n in ch:
            assert 0 <= t < len(sizes) and 1 <= n <= Cs and off >= 0 and off + n <= sizes[t]      # inside ONE tensor, at most C
            seen[t][off:off + n] += 1
        assert all((s == 1).all() for s in seen)                                                  # exactly one cover
        assert ch == sorted(ch)                                                                   # table order, ascending offsets
        assert all(off % Cs == 0 for _, off, _ in ch)                                            # chunks keep a tensor's alignment
        # counting alone (out NULL) agrees
        from babe_amd._lib import lib
        assert lib().babe_opt_chunks((C.c_long * len(sizes))(*sizes), len(sizes), Cs, None, 0) == count


def test_chunk_builder_refusals():
    from babe_amd._lib import lib
    L = lib()
    for sizes, chunk, cap, words in (([5, 9000], 4096, 3, b"cap"), ([5, 0, 7], 4096, None, b"n=0"), ([5, -3], 4096, None, b"n=-3"),
                                     ([5], 0, None, b"chunk"), ([5], 6, None, b"chunk")):
        count, _ = _chunks(sizes, chunk, cap)
        assert count == -1 and words in L.babe_last_error(), (sizes, chunk, cap, L.babe_last_error())
    assert L.babe_opt_chunks(None, 1, 4096, None, 0) == -1 and b"bad arguments" in L.babe_last_error()
    n = (C.c_long * 1)(5)
    assert L.babe_opt_chunks(n, 0, 4096, None, 0) == -1 and b"nt=0" in L.babe_last_error()
    assert _chunks([5, 9000], 4096, 4)[0] == 4                                                    # exactly enough room


def test_launching_entry_points_refuse_bad_arguments_without_a_gpu():
    """Every refusal is made on the host before the first device call: this test runs where there is no device.  The pointers
    are never dereferenced."""
    from babe_amd._lib import lib
    L = lib()
    FAKE = 0x1000
    ERR_ARG = -1

    def step(table=FAKE, chunks=FAKE, nchunks=3, norm=None, max_norm=1.0, lr=1e-3, bc2=0.1, b1=0.9, b2=0.999, eps=1e-8):
        return L.babe_adam_ema_step(table, chunks, nchunks, norm, max_norm, lr, bc2, b1, b2, eps, 0.5, 0.5, None)

    for kw, words in ((dict(table=None), b"null table"), (dict(nchunks=0), b"nchunks=0"), (dict(nchunks=-2), b"nchunks=-2"),
                      (dict(b1=1.0), b"betas"), (dict(b1=-0.1), b"betas"), (dict(b2=1.0), b"betas"), (dict(b2=1.5), b"betas"),
                      (dict(b1=float("nan")), b"betas"), (dict(eps=0.0), b"eps"), (dict(eps=-1e-8), b"eps"),
                      (dict(lr=-1e-3), b"negative learning rate"), (dict(lr=float("nan")), b"learning rate"),
                      (dict(norm=FAKE, max_norm=-1.0), b"max_norm")):
        assert step(**kw) == ERR_ARG and words in L.babe_last_error(), (kw, L.babe_last_error())
    for args, words in (((None, FAKE, 3, FAKE, FAKE), b"null"), ((FAKE, FAKE, 3, None, FAKE), b"null"),
                        ((FAKE, FAKE, 0, FAKE, FAKE), b"nchunks=0"), ((FAKE, FAKE, -1, FAKE, FAKE), b"nchunks=-1")):
        assert L.babe_grad_sqnorm(*args, None) == ERR_ARG and words in L.babe_last_error(), (args, L.babe_last_error())


def test_ema_decay_is_update_emas_scalar():
    """update_ema(dst, src) with dst = 1, src = 0 leaves dst = s: the decay it used, for the ramp's start, its inside, its last
    iteration, its first one past the end and far beyond."""
    from babe_amd.training import ema_decay, update_ema

    class Net(torch.nn.Module):
        def __init__(self, v):
            super().__init__()
            self.w = torch.nn.Parameter(torch.full((3,), v, dtype=torch.float64), requires_grad=False)

    for it, batch in ((0, 2), (1, 2), (4999, 2), (5000, 2), (10 ** 6, 4)):
        ema, net = Net(1.0), Net(0.0)
        update_ema(ema, net, it, batch)
        s = ema_decay(it, batch, 10000, 0.9999)
        assert float(ema.w[0]) == float(s) == min(it * batch / 10000, 0.9999), (it, batch)
        ema, net = Net(1.0), Net(0.0)
        update_ema(ema, net, it, batch, ema_rampup=50, ema_rate=0.9)
        assert float(ema.w[0]) == float(ema_decay(it, batch, 50, 0.9)) == min(it * batch / 50, 0.9)
    assert ema_decay(7, 3) == ema_decay(7, 3, 10000, 0.9999)


def test_constructor_refusals():
    from babe_amd.optim import FusedAdamEMA
    p = [torch.nn.Parameter(torch.zeros(4, 3))]
    FusedAdamEMA(p, lr=1e-3)
    for kw in (dict(weight_decay=0.01), dict(amsgrad=True), dict(maximize=True)):
        with pytest.raises(ValueError, match="plain Adam"):
            FusedAdamEMA(p, lr=1e-3, **kw)
    for bad in (torch.zeros(4, dtype=torch.float64), torch.zeros(4, dtype=torch.bfloat16)):
        with pytest.raises(ValueError, match="float32"):
            FusedAdamEMA([torch.nn.Parameter(bad)], lr=1e-3)
    with pytest.raises(ValueError, match="contiguous"):
        FusedAdamEMA([torch.nn.Parameter(torch.zeros(4, 6).t())], lr=1e-3)
    with pytest.raises(ValueError, match="float32"):
        FusedAdamEMA(p, lr=1e-3, ema_pairs=[(p[0], torch.zeros(4, 3, dtype=torch.float64))])
    with pytest.raises(ValueError, match="EMA tensor"):
        FusedAdamEMA(p, lr=1e-3, ema_pairs=[(p[0], torch.zeros(3, 4))])
    # no CPU fallback: a step over host parameters is refused
    opt = FusedAdamEMA(p, lr=1e-3)
    p[0].grad = torch.ones(4, 3)
    with pytest.raises(ValueError, match="no CPU fallback"):
        opt.step()


def test_state_interchanges_with_torch_adam_on_the_cpu():
    from babe_amd.optim import FusedAdamEMA
    g = torch.Generator().manual_seed(0)
    shapes = [(5, 3), (7,), (2, 2, 2)]

    def params():
        return [torch.nn.Parameter(torch.randn(*s, generator=torch.Generator().manual_seed(i))) for i, s in enumerate(shapes)]

    pa = params()
    adam = torch.optim.Adam(pa, lr=3e-4, betas=(0.8, 0.99), eps=1e-7)
    for p in pa[:2]:                                        # the third has no gradient: no state, as in torch
        p.grad = torch.randn(p.shape, generator=g)
    adam.step()
    sd = adam.state_dict()
    assert sorted(sd["state"]) == [0, 1]
    fused = FusedAdamEMA(params(), lr=1.0)
    fused.load_state_dict(sd)
    back = fused.state_dict()
    assert back["param_groups"] == sd["param_groups"] and back["param_groups"][0]["lr"] == 3e-4
    assert sorted(back["state"]) == [0, 1]
    for i in (0, 1):
        assert set(back["state"][i]) == {"step", "exp_avg", "exp_avg_sq"}
        a, b = sd["state"][i], back["state"][i]
        assert b["step"].dtype == torch.float32 and b["step"].device.type == "cpu" and float(b["step"]) == 1.0
        assert torch.equal(a["step"], b["step"])
        assert torch.equal(a["exp_avg"], b["exp_avg"]) and torch.equal(a["exp_avg_sq"], b["exp_avg_sq"])
        assert a["exp_avg"].abs().sum() > 0
    # the other direction: a fresh FusedAdamEMA's dict has torch.optim.Adam's keys and loads there, and what came back loads too
    fresh = FusedAdamEMA(params(), lr=3e-4, betas=(0.8, 0.99), eps=1e-7)
    ref = torch.optim.Adam(params(), lr=3e-4, betas=(0.8, 0.99), eps=1e-7)
    assert fresh.state_dict()["param_groups"] == ref.state_dict()["param_groups"]
    ref.load_state_dict(back)
    again = ref.state_dict()
    assert again["param_groups"] == sd["param_groups"]
    for i in (0, 1):
        for k in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(again["state"][i][k], sd["state"][i][k])
    for p in ref.param_groups[0]["params"][:2]:             # ... and torch.optim.Adam steps on from it
        p.grad = torch.ones_like(p)
    ref.step()
    assert float(ref.state_dict()["state"][0]["step"]) == 2.0
