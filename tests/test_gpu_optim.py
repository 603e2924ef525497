"""The fused optimizer tail on the GPU (csrc/optim.hip through optim.FusedAdamEMA): norm, clipping, Adam and the EMA element by
element against a float64 restatement on the CPU, with the stock tail (clip_grad_norm_, torch.optim.Adam, training.update_ema on
the GPU) measured in the same units beside it; what must stay untouched; run-to-run bit identity; the step bookkeeping; the NaN
pattern of a non-finite gradient.  Every buffer lies between guard elements.  Needs a MI355X."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
# bars in units of EPS x the operands' magnitudes: m: |m_old| + |g'|, v: v_old + g'^2, ema: |ema_old| + |p_new|,
# p: |p_old| + |update|.  They count the roundings of each expression; where the stock tail's own error is larger, the bar is
# 1.5 x that (final_bar).  Measured values: DESIGN.md, "Training: the fused optimizer tail".
BARS = {"m": 4.0, "v": 4.0, "ema": 4.0, "p": 8.0}
GUARD, FILL = 8, 12345.0
LR, BETAS, ADAM_EPS = 1e-3, (0.9, 0.999), 1e-8
EMA_IT, EMA_BATCH = 1234, 4                                # training.ema_decay -> 0.4936


def final_bar(name, torch_err):
    return max(BARS[name], 1.5 * torch_err)


# ------------------------------------------------------------------------------------------------------------------- inputs
def make_entries(seed=0):
    """CPU float32 inputs: the size list around the chunk size, then one tensor with all-zero g, m, v, one EMA-only entry (no
    gradient), one entry without an EMA tensor and one whose p, g and ema start one element into their allocation."""
    from babe_amd.optim import CHUNK as C
    rng = np.random.RandomState(seed)

    def arr(n, square=False):
        x = rng.randn(n) * 10.0 ** rng.uniform(-4, 2)
        return torch.from_numpy((x * x if square else x).astype(np.float32))

    def entry(n, kind="plain"):
        e = dict(kind=kind, n=n, p=arr(n), g=arr(n), m=arr(n), v=arr(n, square=True), e=arr(n), shift=0)
        if kind == "zero":
            e["g"], e["m"], e["v"] = torch.zeros(n), torch.zeros(n), torch.zeros(n)
        elif kind == "ema_only":
            e["g"] = e["m"] = e["v"] = None
        elif kind == "no_ema":
            e["e"] = None
        elif kind == "offset":
            e["shift"] = 1
        return e

    sizes = [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, C - 1, C, C + 1, 2 * C + 7]
    return [entry(n) for n in sizes] + [entry(261, "zero"), entry(C + 70, "ema_only"), entry(301, "no_ema"), entry(C + 1030, "offset")]


class Guarded:
    """x between GUARD fill elements on each side in a device buffer of its own; shift: the view starts that many elements
    later (4-byte aligned only), with as many more guard elements in front."""

    def __init__(self, x, shift=0):
        n = x.numel()
        self.lo = GUARD + shift
        self.buf = torch.full((self.lo + n + GUARD,), FILL, dtype=torch.float32, device="cuda")
        self.view = self.buf[self.lo:self.lo + n]
        self.view.copy_(x)
        assert self.view.data_ptr() % 16 == (4 * shift) % 16

    def intact(self):
        return bool((self.buf[:self.lo] == FILL).all()) and bool((self.buf[self.lo + self.view.numel():] == FILL).all())


def run_fused(entries, max_norm, k, ema=True):
    """One FusedAdamEMA.step as step number k (the state holds k - 1) on guarded device copies -> per entry the outputs on the CPU,
    the norm, the optimizer and the guards."""
    from babe_amd.optim import FusedAdamEMA
    from babe_amd.training import ema_decay
    bufs, params, pairs = [], [], []
    for e in entries:
        b = {key: Guarded(e[key], e["shift"] if key in ("p", "g", "e") else 0) for key in ("p", "g", "m", "v", "e") if e[key] is not None}
        p = torch.nn.Parameter(b["p"].view)
        if "g" in b:
            p.grad = b["g"].view
        if "e" in b:
            pairs.append((p, b["e"].view))
        bufs.append(b)
        params.append(p)
    opt = FusedAdamEMA(params, lr=LR, betas=BETAS, eps=ADAM_EPS, ema_pairs=pairs)
    for p, b in zip(params, bufs):
        if "g" in b:
            opt.state[p] = {"step": torch.tensor(float(k - 1)), "exp_avg": b["m"].view, "exp_avg_sq": b["v"].view}
    versions = [p._version for p in params]
    opt.step(max_grad_norm=max_norm, ema_s=ema_decay(EMA_IT, EMA_BATCH) if ema else None)
    torch.cuda.synchronize()
    out = [{key: g.view.detach().cpu().clone() for key, g in b.items()} for b in bufs]
    norm = None if opt.last_grad_norm is None else opt.last_grad_norm.cpu()
    return dict(out=out, norm=norm, opt=opt, params=params, bufs=bufs, versions=versions)


def run_torch(entries, max_norm, k):
    """The stock tail on the GPU on the same inputs: clip_grad_norm_, torch.optim.Adam with the same state, training.update_ema."""
    from babe_amd.training import update_ema
    dev = lambda x: None if x is None else x.clone().cuda()
    params = [torch.nn.Parameter(dev(e["p"])) for e in entries]
    emas = [torch.nn.Parameter(dev(e["e"]) if e["e"] is not None else torch.zeros(e["n"], device="cuda"), requires_grad=False)
            for e in entries]
    for p, e in zip(params, entries):
        p.grad = dev(e["g"])
    opt = torch.optim.Adam(params, lr=LR, betas=BETAS, eps=ADAM_EPS)
    for p, e in zip(params, entries):
        if e["g"] is not None:
            opt.state[p] = {"step": torch.tensor(float(k - 1)), "exp_avg": dev(e["m"]), "exp_avg_sq": dev(e["v"])}
    if max_norm is not None:
        torch.nn.utils.clip_grad_norm_(params, max_norm)
    opt.step()
    update_ema(torch.nn.ParameterList(emas), torch.nn.ParameterList(params), EMA_IT, EMA_BATCH)
    torch.cuda.synchronize()
    out = []
    for p, q, e in zip(params, emas, entries):
        o = {"p": p.detach().cpu(), "e": q.detach().cpu() if e["e"] is not None else None}
        if e["g"] is not None:
            o["m"], o["v"] = opt.state[p]["exp_avg"].cpu(), opt.state[p]["exp_avg_sq"].cpu()
        out.append(o)
    return out


def restate(entries, max_norm, k):
    """The formulas of the step in float64 on the fp32 inputs, scalars in double -> per entry the outputs, the magnitudes the
    bars are measured in, and the norm."""
    from babe_amd.training import ema_decay
    sq = sum(float((e["g"].double() ** 2).sum()) for e in entries if e["g"] is not None)
    norm = sq ** 0.5
    coef = 1.0 if max_norm is None else min(1.0, max_norm / (norm + 1e-6))
    b1, b2 = BETAS
    step, bc2s = LR / (1 - b1 ** k), (1 - b2 ** k) ** 0.5
    s = float(ema_decay(EMA_IT, EMA_BATCH))
    out = []
    for e in entries:
        p = e["p"].double()
        o, mag = {}, {}
        if e["g"] is not None:
            g, m, v = coef * e["g"].double(), e["m"].double(), e["v"].double()
            o["m"] = m + (1 - b1) * (g - m)
            o["v"] = b2 * v + (1 - b2) * g * g
            upd = step * o["m"] / (o["v"].sqrt() / bc2s + ADAM_EPS)
            mag["m"], mag["v"], mag["p"] = m.abs() + g.abs(), v + g * g, p.abs() + upd.abs()
            p = p - upd
        o["p"] = p
        if e["e"] is not None:
            o["e"] = e["e"].double() * s + p * (1 - s)
            mag["e"] = e["e"].double().abs() + p.abs()
        out.append((o, mag))
    return out, norm


def errors(got, ref):
    """Worst error per quantity over all entries, in EPS x magnitude (0 / 0 counts as 0, anything / 0 as inf)."""
    worst = {"m": 0.0, "v": 0.0, "ema": 0.0, "p": 0.0}
    for o, (r, mag) in zip(got, ref):
        for key, name in (("m", "m"), ("v", "v"), ("e", "ema"), ("p", "p")):
            if key not in mag or o.get(key) is None:
                continue
            err = (o[key].double() - r[key]).abs()
            ratio = torch.where(err == 0, torch.zeros_like(err), err / (EPS * mag[key]))
            worst[name] = max(worst[name], float(ratio.max()))
    return worst


@pytest.fixture(scope="module")
def entries():
    return make_entries()


@pytest.fixture(scope="module")
def fused_clipped(entries):
    """The step with clipping active (max_norm far below the norm), as step 3 - shared by the tests that only read it."""
    return run_fused(entries, 1.0, 3)


# ------------------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("clip", ["active", "inactive", "off"])
def test_step_against_float64(entries, fused_clipped, clip):
    """Step number 3 (bias corrections 1 - beta^3) with lr = 1e-3, betas = (0.9, 0.999)."""
    max_norm = {"active": 1.0, "inactive": 1e9, "off": None}[clip]
    ref, norm = restate(entries, max_norm, 3)
    assert 100.0 < norm < 1e8                                        # 1.0 clips, 1e9 does not
    fused = fused_clipped if clip == "active" else run_fused(entries, max_norm, 3)
    ef, et = errors(fused["out"], ref), errors(run_torch(entries, max_norm, 3), ref)
    bars = {name: final_bar(name, et[name]) for name in BARS}
    print(f"\nclip {clip}: errors in eps x magnitude   fused {ef}\n   stock tail {et}\n   bars {bars}")
    for name in BARS:
        assert ef[name] <= bars[name], (clip, name, ef[name], bars[name])
    assert all(b["p"].intact() for b in fused["bufs"])
    if clip == "off":
        assert fused["norm"] is None


def test_norm_is_the_float64_norm(entries, fused_clipped):
    _, norm = restate(entries, 1.0, 3)
    got = fused_clipped["norm"]
    assert got.dtype == torch.float64 and got.dim() == 0
    assert abs(float(got) - norm) <= 1e-10 * norm, (float(got), norm)


def test_untouched_where_it_must_be(entries, fused_clipped):
    r = fused_clipped
    for e, o, b, p, v0 in zip(entries, r["out"], r["bufs"], r["params"], r["versions"]):
        for key, g in b.items():
            assert g.intact(), (e["kind"], e["n"], key)                              # guards before and after every buffer
        if e["kind"] == "zero":
            assert torch.equal(o["p"].view(torch.int32), e["p"].view(torch.int32))   # 0 / (0 + eps): p keeps its bits
            assert not o["m"].any() and not o["v"].any()
        elif e["kind"] == "ema_only":
            assert torch.equal(o["p"], e["p"]) and p not in r["opt"].state and p._version == v0
            assert not torch.equal(o["e"], e["e"])
        else:
            assert not torch.equal(o["p"], e["p"]) and p._version > v0                # written, and torch knows
        if e["kind"] == "no_ema":
            assert "e" not in o
        assert torch.equal(o["g"], e["g"]) if e["g"] is not None else "g" not in o   # .grad keeps the unclipped values
    # without ema_s no EMA tensor is written, and an entry with neither gradient nor EMA is not touched at all
    r2 = run_fused(entries, 1.0, 3, ema=False)
    for e, o in zip(entries, r2["out"]):
        if e["e"] is not None:
            assert torch.equal(o["e"], e["e"]), (e["kind"], e["n"])
        if e["kind"] == "ema_only":
            assert torch.equal(o["p"], e["p"])
    assert all(g.intact() for b in r2["bufs"] for g in b.values())


def test_two_runs_give_the_same_bits(entries, fused_clipped):
    again = run_fused(entries, 1.0, 3)
    assert torch.equal(again["norm"].view(torch.int64), fused_clipped["norm"].view(torch.int64))
    for a, b in zip(again["out"], fused_clipped["out"]):
        assert set(a) == set(b)
        for key in a:
            assert torch.equal(a[key].view(torch.int32), b[key].view(torch.int32)), key


def test_three_steps_bookkeeping_and_third_step(entries):
    """Three real steps from an empty state with new gradients each time: `step` counts them, the parameter without a gradient
    never gets a state, and the third step equals the restatement at k = 3 on the state the second one left."""
    from babe_amd.optim import FusedAdamEMA
    from babe_amd.training import ema_decay
    rng = torch.Generator().manual_seed(7)
    params = [torch.nn.Parameter(e["p"].clone().cuda()) for e in entries]
    emas = [e["e"].clone().cuda() if e["e"] is not None else None for e in entries]
    opt = FusedAdamEMA(params, lr=LR, betas=BETAS, eps=ADAM_EPS, ema_pairs=[(p, q) for p, q in zip(params, emas) if q is not None])
    before = None
    for k in (1, 2, 3):
        grads = [None if e["g"] is None else torch.randn(e["n"], generator=rng) * float(e["g"].abs().max() + 1e-3) for e in entries]
        for p, g in zip(params, grads):
            p.grad = None if g is None else g.cuda()
        if k == 3:
            torch.cuda.synchronize()
            before = [dict(kind=e["kind"], n=e["n"], p=p.detach().cpu().clone(), g=g, e=None if q is None else q.cpu().clone(),
                           m=opt.state[p]["exp_avg"].cpu().clone() if g is not None else None,
                           v=opt.state[p]["exp_avg_sq"].cpu().clone() if g is not None else None)
                      for e, p, q, g in zip(entries, params, emas, grads)]
        opt.step(max_grad_norm=1.0, ema_s=ema_decay(EMA_IT, EMA_BATCH))
    torch.cuda.synchronize()
    for e, p in zip(entries, params):
        if e["g"] is None:
            assert p not in opt.state
        else:
            st = opt.state[p]
            assert float(st["step"]) == 3.0 and st["step"].device.type == "cpu" and st["step"].dtype == torch.float32
    sd = opt.state_dict()
    assert len(sd["state"]) == sum(e["g"] is not None for e in entries)
    ref, _ = restate(before, 1.0, 3)
    got = [{"p": p.detach().cpu(), "e": None if q is None else q.cpu(),
            "m": opt.state[p]["exp_avg"].cpu() if p in opt.state else None,
            "v": opt.state[p]["exp_avg_sq"].cpu() if p in opt.state else None} for p, q in zip(params, emas)]
    ef, et = errors(got, ref), errors(run_torch(before, 1.0, 3), ref)
    print(f"\nthird of three steps: fused {ef}\n   stock tail {et}")
    for name in BARS:
        assert ef[name] <= final_bar(name, et[name]), (name, ef[name], et[name])
    # the same bias corrections at another step count would miss by far: k = 2 moves p by a different step size
    wrong, _ = restate(before, 1.0, 2)
    assert errors(got, wrong)["p"] > 1e3


def test_non_finite_gradient_gives_torchs_nan_pattern(entries):
    bad = [dict(e) for e in entries]
    i = next(j for j, e in enumerate(bad) if e["n"] == 257)
    bad[i]["g"] = bad[i]["g"].clone()
    bad[i]["g"][100] = float("inf")
    for max_norm in (1.0, None):
        fused, stock = run_fused(bad, max_norm, 3), run_torch(bad, max_norm, 3)
        if max_norm is not None:
            assert torch.isinf(fused["norm"])
        nans = 0
        for e, a, b in zip(bad, fused["out"], stock):
            for key in ("p", "m", "v", "e"):
                if b.get(key) is not None:
                    assert torch.equal(torch.isnan(a[key]), torch.isnan(b[key])), (max_norm, e["n"], key)
                    nans += int(torch.isnan(a[key]).sum())
        # clipped: coef = max_norm / inf = 0 and 0 * inf = NaN in g', so m, v and p of that element; unclipped: m = v = inf, and
        # p = p - step * (inf / inf)
        assert torch.isnan(fused["out"][i]["p"][100]) and nans >= 1
        assert bool(torch.isnan(fused["out"][i]["m"][100])) == (max_norm is not None)
