"""ctypes view of a library-built denoiser (csrc/dn_engine.hip: babe_denoiser_load and friends) - what a host without Python holds
instead of a MultiStage_denoise and a DenoiserPrepass.  Used by tests/test_gpu_dn_library.py, tools/denoiser_library_bench.py and
long_file.restore_file_library only: the Python flows keep their own engine."""
import ctypes as C

import numpy as np
import torch

from .._cabi import DenoiserSummary, SincTable
from .._lib import BabeHipError, check, lib, ptr, stream


class LibraryDenoiser:
    """babe_denoiser_load(path) on the current device and stream; `close()` (or garbage collection) destroys it."""

    def __init__(self, path):
        self.handle = lib().babe_denoiser_load(str(path).encode(), stream())
        if not self.handle:
            raise BabeHipError("babe_denoiser_load: " + lib().babe_last_error().decode())
        self._ws = {}

    def close(self):
        if getattr(self, "handle", None):
            lib().babe_denoiser_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def info(self):
        s = DenoiserSummary()
        check(lib().babe_denoiser_info(self.handle, C.byref(s)), "denoiser_info")
        return s

    def _get(self, k):
        """The leaves DenoiserPrepass._get serves, from the handle."""
        i = self.info
        return {"sample_rate_denoiser": i.sample_rate, "stft_win_size": i.win, "stft_hop_size": i.hop, "num_stages": i.num_stages}[k]

    def workspace(self, need, device, key):
        """A cached byte buffer of at least `need` bytes (one per key: two streams take two keys)."""
        if need < 0:
            check(int(need), "workspace_bytes")
        w = self._ws.get(key)
        if w is None or w.numel() < need:
            w = self._ws[key] = torch.empty(max(need, 1), dtype=torch.uint8, device=device)
        return w

    def forward(self, X, ws=None, ws_bytes=None):
        """MultiStage_denoise.forward: X [B, 2, T, F] -> (pred2, pred1), or pred1 for one stage."""
        X = X.contiguous().float()
        B, _, T, F = X.shape
        L = lib()
        if ws is None:
            ws = self.workspace(L.babe_denoiser_workspace_bytes(self.handle, B, T, F), X.device, "fwd")
        two = self.info.num_stages > 1
        p1, p2 = torch.empty_like(X), (torch.empty_like(X) if two else None)
        check(L.babe_denoiser_fwd(self.handle, ptr(X), ptr(p2), ptr(p1), ptr(ws), ws.numel() if ws_bytes is None else ws_bytes, B, T, F,
                                  stream(X)), "denoiser_fwd")
        return (p2, p1) if two else p1

    __call__ = forward

    def apply_denoiser(self, x, ws=None, ws_bytes=None):
        """DenoiserPrepass.apply_denoiser: x [B, n] at the denoiser's rate -> [B, n]."""
        x = x.contiguous().float()
        B, n = x.shape
        L = lib()
        if ws is None:
            ws = self.workspace(L.babe_denoise_signal_workspace_bytes(self.handle, B, n), x.device, "signal")
        out = torch.empty_like(x)
        check(L.babe_denoise_signal(self.handle, ptr(x), x.stride(0), ptr(out), out.stride(0), B, n, ptr(ws),
                                    ws.numel() if ws_bytes is None else ws_bytes, stream(x)), "denoise_signal")
        return out


def sinc_table(orig_freq, new_freq, device, python=False):
    """(SincTable, tensors to keep alive) of one conversion on `device`: the library's own builder (babe_resample_sinc_table),
    or - python=True - the table babe_amd/resample.py builds, for a bit-exact comparison with the Python flow."""
    t = SincTable()
    if python:
        from ..resample import _table
        kern, krange, t.width, t.orig, t.new_ = _table(orig_freq, new_freq, 6, 0.99, device)
    else:
        w, o, nw = C.c_int(), C.c_int(), C.c_int()
        size = lib().babe_resample_sinc_table_size(int(orig_freq), int(new_freq), C.byref(w), C.byref(o), C.byref(nw))
        if size < 0:
            check(int(size), "resample_sinc_table_size")
        k, kr = np.empty(size, np.float32), np.empty(2 * nw.value, np.int32)
        check(lib().babe_resample_sinc_table(int(orig_freq), int(new_freq), k.ctypes.data, kr.ctypes.data), "resample_sinc_table")
        kern, krange = torch.from_numpy(k).to(device), torch.from_numpy(kr).to(device)
        t.width, t.orig, t.new_ = w.value, o.value, nw.value
    t.kernel, t.krange = ptr(kern), ptr(krange)
    return t, (kern, krange)
