"""ctypes binding of libbabe_hip.so (the C-ABI declared in include/babe_hip.h).

There is no CPU fallback: if the library is missing or a call fails this raises.
"""
import ctypes as C
import os

import torch

from ._cabi import ConvArgs, bind  # noqa: F401  (ConvArgs: imported from here by tests and tools)

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.environ.get("BABE_HIP_LIB") or os.path.join(_HERE, "libbabe_hip.so")
_lib = None


class BabeHipError(RuntimeError):
    pass


def lib():
    """The loaded library with every entry point of _cabi.SIGS declared (and no other babe_* name)."""
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise BabeHipError(
                f"{_LIB_PATH} not found: build it with `python -m babe_amd.build` (there is no CPU fallback)")
        _lib = bind(_LIB_PATH)
    return _lib


def prof_slot_names():
    L = lib()
    return [L.babe_prof_slot_name(i).decode() for i in range(L.babe_prof_nslots())]


_prof_on = False

def prof_enable(on):
    """Measurement hook (include/babe_hip.h): HIP-event timing of every launch, tallied per kernel slot."""
    global _prof_on
    _prof_on = bool(on)
    lib().babe_prof_enable(int(bool(on)))


def prof_enabled():
    """True while the measurement hook is on.  Asks the LIBRARY (babe_prof_enable(-1) = query): another binding may have
    switched it on."""
    return bool(_prof_on or (lib().babe_prof_enable(-1) == 1))


def prof_read():
    """{slot name: dict(ms, bytes, flops, exec_flops, launches)} since the last read (waits for the GPU); resets."""
    L = lib()
    n = L.babe_prof_nslots()
    D, Lg = (C.c_double * n), (C.c_long * n)
    ms, by, fl, ex, nl = D(), D(), D(), D(), Lg()
    check(L.babe_prof_read(ms, by, fl, ex, nl), "prof_read")
    return {name: dict(ms=ms[i], bytes=by[i], flops=fl[i], exec_flops=ex[i], launches=nl[i])
            for i, name in enumerate(prof_slot_names())}


def prof_timeline():
    """Per-launch records pending since the last prof_read() - call BEFORE it: dict of numpy arrays t0_ms, t1_ms (relative to
    the first record), slot (index into prof_slot_names()), lane (stream index), flops.  Waits for the GPU."""
    import numpy as np
    L = lib()
    n = int(L.babe_prof_pending())
    t0, t1, fl = np.zeros(n), np.zeros(n), np.zeros(n)
    sl, ln = np.zeros(n, np.int32), np.zeros(n, np.int32)
    as_p = lambda a: a.ctypes.data_as(C.c_void_p)
    m = L.babe_prof_timeline(as_p(t0), as_p(t1), as_p(sl), as_p(ln), as_p(fl), n)
    if m < 0:
        raise BabeHipError(f"prof_timeline failed ({m}): {L.babe_last_error().decode()}")
    return dict(t0_ms=t0[:m], t1_ms=t1[:m], slot=sl[:m], lane=ln[:m], flops=fl[:m])


def dispatch_counts(reset=False):
    """Always-on launch counters per slot: which kernel each conv call really took (wino4 / wino2 / direct / bf16)."""
    L = lib()
    n = L.babe_prof_nslots()
    cnt = (C.c_long * n)()
    L.babe_prof_dispatch_counts(cnt, int(reset))
    return {name: cnt[i] for i, name in enumerate(prof_slot_names())}


def check(rc, what=""):
    if rc != 0:
        raise BabeHipError(f"{what} failed ({rc}): {lib().babe_last_error().decode()}")


def workspace(cache, key, nbytes, device, what, keep_all=False):
    """The caller-owned workspace of a library entry point, as a uint8 tensor kept in the dict `cache` under `key`: the latest key
    only, or with keep_all one buffer per key.  nbytes: a callable returning what babe_<what>_workspace_bytes says, asked when
    the key is new; a negative size raises with the library's message."""
    ws = cache.get(key)
    if ws is None:
        n = nbytes()
        if n < 0:
            raise BabeHipError(f"{what}_workspace_bytes failed ({n}): {lib().babe_last_error().decode()}")
        if not keep_all:
            cache.clear()
        ws = cache[key] = torch.empty(n, device=device, dtype=torch.uint8)
    return ws


def ptr(t):
    if t is None:
        return None
    assert t.is_cuda, "babe_amd ops need device tensors (no CPU fallback)"
    return t.data_ptr()


def stream(t=None):
    """HIP stream the next launch goes to: the current stream OF THE DEVICE the operands live on (`t`: a tensor or a
    torch.device).  The library never calls hipSetDevice; launching device-1 pointers on device 0's stream faults, so
    multi-device hosts must either pass `t` or run under torch.cuda.device(...) as the network/sampler entry points do."""
    if t is None:
        return torch.cuda.current_stream().cuda_stream
    return torch.cuda.current_stream(t.device if torch.is_tensor(t) else t).cuda_stream
