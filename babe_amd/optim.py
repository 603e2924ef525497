"""The tail of a training iteration as HIP kernels (csrc/optim.hip): the gradients' L2 norm, clipping, Adam and the EMA of the
weights in three launches over all parameter tensors, in place of clip_grad_norm_ + torch.optim.Adam.step() + training.update_ema
(three element-wise torch passes per tensor).

    opt = FusedAdamEMA(net.parameters(), lr=2e-4, betas=(0.9, 0.999), eps=1e-8, ema_pairs=zip(net.parameters(), ema.parameters()))
    loss.backward()
    opt.step(max_grad_norm=1.0, ema_s=training.ema_decay(it, batch, ema_rampup, ema_rate))

The state is torch.optim.Adam's - per parameter `step` (a CPU float32 scalar), `exp_avg`, `exp_avg_sq`; state_dict() loads into
torch.optim.Adam and the other way round, so a checkpoint does not say which of the two wrote it.  The formulas are Adam's
(amsgrad, weight decay and maximize are refused): the moments in torch's fp32 operations, the parameter update and the EMA in
double from them and rounded once, so parameters agree with torch's to a few units in the last place, not bit for bit.  One difference from clip_grad_norm_: `.grad` is NOT rewritten
with the clipped values - the coefficient is applied in registers.
There is no CPU fallback: step() refuses parameters that are not on a GPU.  (The constructor accepts them, so that optimizer
state can be loaded, converted and saved on a machine without one.)"""
import ctypes as C

import numpy as np
import torch

from ._cabi import OptChunk, OptTensor

CHUNK = 8192                      # elements per workgroup: 8 float4 per thread and array
_ROW = C.sizeof(OptTensor) // 8   # the table as int64 words: p, g, m, v, ema, n


class FusedAdamEMA(torch.optim.Optimizer):
    """Adam with the gradient clipping before it and the weights' EMA after it in the same pass.

    params, lr, betas, eps: as torch.optim.Adam (parameter groups included; weight_decay != 0, amsgrad and maximize raise
    ValueError, and so does a parameter that is not contiguous float32).
    ema_pairs: iterable of (parameter, EMA tensor of the same shape, contiguous float32 on the same device), or None; attach_ema()
    sets it later.  A pair whose parameter the optimizer does not own is averaged too.

    step(max_grad_norm=None, ema_s=None): max_grad_norm clips the global L2 norm as clip_grad_norm_(params, max_grad_norm) would
    (last_grad_norm: that norm as a 0-dim float64 device tensor, None without clipping; nothing waits for the GPU);
    ema_s: ema = ema * ema_s + p_new * (1 - ema_s) for every attached pair, None: the EMA tensors are left alone.
    A parameter whose .grad is None is skipped as torch.optim.Adam skips it (no state, `step` not advanced) but still averaged.
    Every tensor the kernel writes gets its version counter advanced, so whoever caches derived data (the network's packed conv
    images) sees the change."""

    fused_tail = True             # training.train_step: clipping and the EMA belong to step()

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, ema_pairs=None, weight_decay=0, amsgrad=False, maximize=False):
        if weight_decay != 0 or amsgrad or maximize:
            raise ValueError("FusedAdamEMA implements plain Adam: weight_decay, amsgrad and maximize are not supported")
        if not 0.0 <= lr:
            raise ValueError(f"invalid learning rate {lr}")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"invalid betas {betas}")
        if not 0.0 < eps:
            raise ValueError(f"invalid eps {eps}")
        # the defaults - and with them the keys of every param_group - are torch.optim.Adam's own: state_dict()s interchange
        defaults = dict(torch.optim.Adam([torch.zeros(1)], lr=lr, betas=betas, eps=eps).defaults)
        super().__init__(params, defaults)
        for group in self.param_groups:
            for p in group["params"]:
                self._check_tensor(p, "parameter")
        self._ema = {}
        self.last_grad_norm = None
        self._chunks = {}             # entry sizes -> (device chunk table, chunk count)
        self._slots = None            # two (pinned host table, device table, event) sets, used in turn
        self._turn = 0
        self._partials = self._norm = None
        if ema_pairs is not None:
            self.attach_ema(ema_pairs)

    @staticmethod
    def _check_tensor(t, what):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError(f"FusedAdamEMA: a {what} of dtype {t.dtype}, contiguous={t.is_contiguous()} (contiguous float32 only)")

    def attach_ema(self, pairs):
        """(parameter, EMA tensor) pairs for step(ema_s=...); replaces earlier ones."""
        self._ema = {}
        for p, e in pairs:
            self._check_tensor(e, "EMA tensor")
            if e.shape != p.shape or e.device != p.device:
                raise ValueError(f"FusedAdamEMA: EMA tensor {tuple(e.shape)} on {e.device} for a parameter {tuple(p.shape)} on {p.device}")
            self._ema[p] = e

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        g = self.param_groups[-1]
        if g.get("weight_decay", 0) != 0 or g.get("amsgrad", False) or g.get("maximize", False):
            raise ValueError("FusedAdamEMA implements plain Adam: weight_decay, amsgrad and maximize are not supported")

    def load_state_dict(self, state_dict):
        """torch.optim.Adam's or this class's.  `step` comes back to the host as a float32 scalar wherever the checkpoint was
        mapped to: step() reads it on the host and must not wait for the GPU."""
        super().load_state_dict(state_dict)
        for g in self.param_groups:
            if g.get("weight_decay", 0) != 0 or g.get("amsgrad", False) or g.get("maximize", False):
                raise ValueError("FusedAdamEMA implements plain Adam: weight_decay, amsgrad and maximize are not supported")
        for st in self.state.values():
            if "step" in st:
                k = st["step"]
                st["step"] = k.detach().to("cpu", torch.float32) if torch.is_tensor(k) else torch.tensor(float(k), dtype=torch.float32)

    # ---------------------------------------------------------------- the table
    def _upload(self, rows, device, stream):
        """rows [nt][6] int64 -> a device table.  Gradients are new allocations every step, so the table is rewritten every
        step: filled in pinned host memory and copied asynchronously on the step's stream.  Two sets used in turn, each with an
        event recorded behind its copy - a host table is not overwritten while a copy may still read it."""
        nt = len(rows)
        if self._slots is None or self._slots[0][0].shape[0] < nt or self._slots[0][1].device != device:
            cap = max(nt, 64)
            self._slots = [(torch.empty(cap, _ROW, dtype=torch.int64).pin_memory(),
                            torch.empty(cap, _ROW, dtype=torch.int64, device=device), torch.cuda.Event()) for _ in range(2)]
            self._used = [False, False]
        host, dev, ev = self._slots[self._turn]
        if self._used[self._turn]:
            ev.synchronize()                   # the copy of two steps ago: over long before
        host.numpy()[:nt] = rows
        dev[:nt].copy_(host[:nt], non_blocking=True)
        ev.record(stream)
        self._used[self._turn] = True
        self._turn ^= 1
        return dev

    def _chunk_table(self, sizes, device):
        """The chunk table of entries with these sizes, on the device (built once per distinct list)."""
        from ._lib import BabeHipError, lib
        hit = self._chunks.get(sizes)
        if hit is None:
            L = lib()
            n = (C.c_long * len(sizes))(*sizes)
            count = L.babe_opt_chunks(n, len(sizes), CHUNK, None, 0)
            if count < 0:
                raise BabeHipError(f"opt_chunks failed: {L.babe_last_error().decode()}")
            out = (OptChunk * count)()
            if L.babe_opt_chunks(n, len(sizes), CHUNK, out, count) != count:
                raise BabeHipError(f"opt_chunks failed: {L.babe_last_error().decode()}")
            host = torch.from_numpy(np.frombuffer(out, dtype=np.int64).copy())
            if len(self._chunks) >= 8:
                self._chunks.clear()
            hit = self._chunks[sizes] = (host.to(device), count)
        return hit

    # ---------------------------------------------------------------- step
    @torch.no_grad()
    def step(self, closure=None, max_grad_norm=None, ema_s=None):
        from ._lib import check, lib
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        ema = self._ema if ema_s is not None else {}
        # launches: parameters that share the group's scalars and the step count; EMA-only entries ride with the first
        launches, ema_only, seen = {}, [], set()
        for gi, group in enumerate(self.param_groups):
            for p in group["params"]:
                seen.add(p)
                if p.grad is None:
                    if p in ema:
                        ema_only.append(p)
                    continue
                if p.grad.is_sparse:
                    raise RuntimeError("FusedAdamEMA does not support sparse gradients")
                st = self.state[p]
                if len(st) == 0:
                    st["step"] = torch.tensor(0.0, dtype=torch.float32)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["step"] += 1
                launches.setdefault((gi, float(st["step"])), []).append(p)
        ema_only += [p for p in ema if p not in seen]
        self.last_grad_norm = None
        if not launches and not ema_only:
            return loss
        order = [(key, ps) for key, ps in launches.items()]
        if ema_only:
            if order:
                order[0] = (order[0][0], order[0][1] + ema_only)
            else:
                order = [(None, ema_only)]
        rows, sizes, written = [], [], []
        device = order[0][1][0].device
        for _, ps in order:
            for p in ps:
                g = p.grad
                e = ema.get(p)
                if p.device != device or device.type != "cuda":
                    raise ValueError(f"FusedAdamEMA: parameters on {p.device} and {device} (one GPU; there is no CPU fallback)")
                if g is not None:
                    st = self.state[p]
                    m, v = st["exp_avg"], st["exp_avg_sq"]
                    if g.dtype != torch.float32 or not g.is_contiguous() or g.device != device:
                        raise ValueError(f"FusedAdamEMA: a gradient of dtype {g.dtype}, contiguous={g.is_contiguous()} on {g.device}")
                    for t in (m, v):
                        self._check_tensor(t, "moment")
                        if t.device != device or t.numel() != p.numel():
                            raise ValueError("FusedAdamEMA: optimizer state does not match its parameter")
                    rows.append((p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), e.data_ptr() if e is not None else 0, p.numel()))
                    written += [p, m, v]
                else:
                    rows.append((p.data_ptr(), 0, 0, 0, e.data_ptr(), p.numel()))
                if e is not None:
                    written.append(e)
                sizes.append(p.numel())
        sizes = tuple(sizes)
        if 0 in sizes:
            raise ValueError("FusedAdamEMA: a parameter without elements")
        L = lib()
        with torch.cuda.device(device):
            stream = torch.cuda.current_stream(device)
            s = stream.cuda_stream
            chunks, nchunks = self._chunk_table(sizes, device)
            table = self._upload(rows, device, stream)
            norm_ptr = None
            if max_grad_norm is not None:
                if self._partials is None or self._partials.numel() < nchunks or self._partials.device != device:
                    self._partials = torch.empty(nchunks, dtype=torch.float64, device=device)
                # a fresh scalar per step: last_grad_norm stays what it was when a later step runs
                self.last_grad_norm = torch.empty((), dtype=torch.float64, device=device)
                norm_ptr = self.last_grad_norm.data_ptr()
                check(L.babe_grad_sqnorm(table.data_ptr(), chunks.data_ptr(), nchunks, self._partials.data_ptr(), norm_ptr, s),
                      "grad_sqnorm")
            es, e1 = (float(ema_s), 1.0 - float(ema_s)) if ema_s is not None else (1.0, 0.0)
            c0 = t0 = 0
            for key, ps in order:
                t1 = t0 + len(ps)
                c1 = c0 + sum(-(-n // CHUNK) for n in sizes[t0:t1])
                if key is None:                                   # EMA-only entries alone: Adam's scalars are not used
                    lr_bc1, bc2s, b1, b2, eps = 0.0, 1.0, 0.0, 0.0, 1.0
                else:
                    group, k = self.param_groups[key[0]], key[1]
                    b1, b2 = group["betas"]
                    lr_bc1 = float(group["lr"]) / (1 - b1 ** k)
                    bc2s = (1 - b2 ** k) ** 0.5
                    eps = group["eps"]
                check(L.babe_adam_ema_step(table.data_ptr(), chunks.data_ptr() + c0 * C.sizeof(OptChunk), c1 - c0, norm_ptr,
                                           float(max_grad_norm) if max_grad_norm is not None else 0.0, lr_bc1, bc2s, b1, b2, eps,
                                           es, e1, s), "adam_ema_step")
                c0, t0 = c1, t1
        # the kernel wrote behind torch's back: advance the version counters (the network repacks its conv images on a new
        # parameter version; without this it would go on training with stale packed weights)
        torch.autograd.graph.increment_version(written)
        return loss
