"""Cases and float64 references of the length-L real FFT tests (tests/test_fft_cases_cpu.py pins the references on the CPU,
tests/test_gpu_fft.py runs the kernels, and its child process under BABE_FFT_REAL=0 runs `python tests/fft_cases.py`).

The transform under test (csrc/fft_mixed.hip, babe_rfft_mixed; RealFFT in babe_amd/cqt.py): L = N1 * N2, planar spectrum
[B][2][KX], KX = K2 * N1, bin k = k1 + N1 k2 in natural order.
  forward   : spec[0][k] + i spec[1][k] = X[k] = sum_n x[n] e^{-2 pi i k n / L} for EVERY k < KX (also the bins above L/2)
  transpose : x[n] = Re sum_{k < KX} (G[0][k] + i G[1][k]) e^{+2 pi i k n / L}   (G zero above L/2, as RealFFT.rfft_T asks)
"""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

RADICES = (2, 3, 4, 5, 7, 11, 13, 23)
BAR = 5e-6            # the project's bar for the mixed-radix transform (tests/test_gpu_cqt.py, set at L = 368368)
GUARD = 64            # floats of canary on either side of every device buffer of a direct C-ABI call

# (N1, N2, radices of N1, radices of N2, also run with K2 = N2, what the row reaches)
CASES = [
    (2, 3, (2,), (3,), False, "single-pass radices 2 and 3; N < 7; fewer columns than one tile"),
    (4, 4, (4,), (4,), True, "radix-4 single pass; even Nyquist row"),
    (5, 7, (5,), (7,), True, "odd x odd, L odd (no Nyquist); odd-N1 mirror bounds"),
    (13, 23, (13,), (23,), False, "the two largest radices as single passes"),
    (23, 11, (23,), (11,), False, "N1 > N2"),
    (8, 16, (4, 2), (4, 4), False, "twiddled second pass; radix 2 after 4"),
    (9, 25, (3, 3), (5, 5), False, "repeated odd radices"),
    (15, 14, (3, 5), (2, 7), False, "N2 = exactly one packed tile of 14 real columns"),
    (14, 15, (2, 7), (3, 5), True, "packed tile plus one lone column (oka && !okb)"),
    (12, 35, (4, 3), (5, 7), False, "N2 = 2*14 + 7: last packed tile half full; stage-2 N1/2+1 = 7 = exactly one tile"),
    (26, 46, (2, 13), (2, 23), False, "radices 13 and 23 as later (twiddled) passes"),
    (30, 462, (2, 3, 5), (2, 3, 7, 11), False, "33 packed tiles: the tile bijection past the first padded block of 32"),
    (450, 462, (2, 3, 3, 5, 5), (2, 3, 7, 11), False, "more than 32 tiles in stage 2 as well; five radices"),
    (2, 810, (2,), (2, 3, 3, 3, 3, 5), False, "six radices, the maximum count"),
    (2, 1056, (2,), (4, 4, 2, 3, 11), False, "largest N below RealFFT's 1077; 126 KB LDS opt-in"),
    (2, 1365, (2,), (3, 5, 7, 13), False, "largest N the LDS check admits: 163800 of 163840 bytes"),
]


def case_id(c):
    return f"{c[0]}x{c[1]}"


def case_by_id(name):
    return next(c for c in CASES if case_id(c) == name)


def k2_of(N1, N2):
    return ((N1 * N2) // 2) // N1 + 1


def runs():
    """Every (case, K2) of the table: K2 = (L//2)//N1 + 1, and K2 = N2 for the rows that ask for it."""
    out = []
    for c in CASES:
        out.append((c, k2_of(c[0], c[1])))
        if c[4] and k2_of(c[0], c[1]) != c[1]:
            out.append((c, c[1]))
    return out


def pass_positions():
    """(radices that occur as a first pass (Ns = 1), radices that occur as a later, twiddled pass) over the table."""
    first, later = set(), set()
    for c in CASES:
        for rad in (c[2], c[3]):
            first.add(rad[0])
            later.update(rad[1:])
    return first, later


# ----------------------------------------------------------------------------- tables, inputs, references (CPU)
def _unit(num, den):
    """exp(-2 pi i num / den) as float64 [..., 2], the angle reduced in integers first."""
    ang = 2.0 * np.pi * (np.asarray(num, dtype=np.int64) % den).astype(np.float64) / den
    return np.stack([np.cos(ang), -np.sin(ang)], -1)


def tables(N1, N2):
    """w1 [N1][2], w2 [N2][2], tw [N1][N2][2]: computed in float64, rounded to float32 (what RealFFT builds)."""
    w1, w2 = _unit(np.arange(N1), N1), _unit(np.arange(N2), N2)
    tw = _unit(np.arange(N1)[:, None] * np.arange(N2)[None, :], N1 * N2)
    return tuple(torch.tensor(a, dtype=torch.float32).contiguous() for a in (w1, w2, tw))


def inputs(L, KX, B, seed):
    """x [B][L] and G [B][2][KX] (zero above L/2), seeded."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, L, generator=g)
    G = torch.zeros(B, 2, KX)
    n = min(L // 2 + 1, KX)
    G[:, :, :n] = torch.randn(B, 2, n, generator=g)
    return x, G


def ref_forward(x, KX):
    """[B][KX] complex128: X[k], k < KX."""
    return torch.fft.fft(x.double(), dim=-1)[:, :KX]


def ref_transpose(G, L):
    """[B][L] float64: L * ifft(Z).real with Z[k] = Gr[k] + i Gi[k] for k < KX, zero above."""
    B, _, KX = G.shape
    Z = torch.zeros(B, L, dtype=torch.complex128)
    Z[:, :KX] = torch.complex(G[:, 0].double(), G[:, 1].double())
    return L * torch.fft.ifft(Z, dim=-1).real


def forward_matrix(L, KX):
    """The forward map as an explicit float64 matrix M [L][2 KX]: x @ M = (Re X[0..KX), Im X[0..KX))."""
    kn = (np.arange(L, dtype=np.int64)[:, None] * np.arange(KX, dtype=np.int64)[None, :]) % L
    ang = 2.0 * np.pi * kn.astype(np.float64) / L
    return torch.from_numpy(np.concatenate([np.cos(ang), -np.sin(ang)], 1))


def planar(X):
    """complex [B][K] -> planar float64 [B][2][K]."""
    return torch.stack([X.real, X.imag], 1)


def row_err(got, ref):
    """max|got - ref| / max|ref| per batch row (complex magnitudes for spectra): the metric of tests/test_gpu_cqt.py.
    NaN (an output the kernel did not write, or one computed from a canary) stays NaN and fails every `<`."""
    d = (got - ref).abs().reshape(got.shape[0], -1)
    return [float(d[b].max() / ref[b].abs().max()) if not bool(torch.isnan(d[b]).any()) else float("nan")
            for b in range(got.shape[0])]


def as_complex(spec):
    return torch.complex(spec[:, 0].double().cpu(), spec[:, 1].double().cpu())


def adjoint_gap(spec, G, x, xt, Xref, xtref):
    """(|<spec, G> - <x, xt>|, its bar).  Both products are summed in float64 from the float32 results.  The element-wise
    tests bound the 2-norm error of either result by BAR times the 2-norm of its reference (a rounding error of an FFT is
    proportional to the input's 2-norm and spread evenly over the outputs); <Xref, G> = <x, xtref> exactly, so by
    Cauchy-Schwarz the two products differ by at most BAR (|Xref| |G| + |x| |xtref|).  No absolute slack."""
    lhs = float((spec.double().cpu() * G.double()).sum())
    rhs = float((x.double() * xt.double().cpu()).sum())
    bar = BAR * (float(planar(Xref).norm()) * float(G.double().norm()) + float(x.double().norm()) * float(xtref.norm()))
    return abs(lhs - rhs), bar


# ----------------------------------------------------------------------------- the direct C-ABI call (GPU)
class Guarded:
    """A device buffer of n floats between two canaries of GUARD floats.  Inputs lie between NaNs (a read outside the buffer
    poisons the result), outputs are pre-filled with NaN (a bin the kernel does not write fails the comparison) between
    canaries that must come back untouched."""

    def __init__(self, n, fill=float("nan"), canary=float("nan"), src=None):
        self.n = n
        self.buf = torch.full((n + 2 * GUARD,), fill, device="cuda")
        self.canary = canary
        self.buf[:GUARD] = canary
        self.buf[GUARD + n:] = canary
        if src is not None:
            self.mid.copy_(src.reshape(-1))

    @property
    def mid(self):
        return self.buf[GUARD:GUARD + self.n]

    def canaries_intact(self):
        edge = torch.cat([self.buf[:GUARD], self.buf[GUARD + self.n:]]).cpu()
        want = torch.full_like(edge, self.canary)
        return bool(torch.equal(edge.view(torch.int32), want.view(torch.int32)))


def mixed_call(src, N1, N2, K2, rad1, rad2, direction, raw=False, **bad):
    """babe_rfft_mixed the way RealFFT._mixed calls it.  direction 0: src = x [B][L] -> spec [B][2][K2 N1]; 1: src = G -> x.
    Returns (result on the CPU, return code); raises AssertionError when a canary was written.  `bad`: overrides for the
    refusal tests (rad1, rad2, nrad1, nrad2, K2_arg, work=None)."""
    from babe_amd._lib import lib, stream
    B, L, KX = src.shape[0], N1 * N2, K2 * N1
    w1, w2, tw = (Guarded(t.numel(), src=t) for t in tables(N1, N2))
    inp = Guarded(src.numel(), src=src)
    work = Guarded(B * 2 * L)
    # 7.0: a value no transform of these inputs produces, so an untouched output is recognisable in the refusal tests
    out = Guarded(B * 2 * max(KX, 1) if direction == 0 else B * L, fill=float("nan") if not raw else 7.0, canary=-3.0)
    r1, r2 = bad.get("rad1", rad1), bad.get("rad2", rad2)
    r1c, r2c = (C.c_int * len(r1))(*r1), (C.c_int * len(r2))(*r2)
    p = lambda gd: gd.mid.data_ptr()
    rc = lib().babe_rfft_mixed(p(inp) if direction == 0 else None, p(out) if direction == 0 else None,
                               p(inp) if direction == 1 else None, p(out) if direction == 1 else None,
                               None if "work" in bad else p(work), B, N1, N2, bad.get("K2_arg", K2), r1c, bad.get("nrad1", len(r1)),
                               r2c, bad.get("nrad2", len(r2)), p(w1), p(w2), p(tw), direction, stream())
    torch.cuda.synchronize()
    for name, gd in (("input", inp), ("work", work), ("output", out), ("w1", w1), ("w2", w2), ("tw", tw)):
        assert gd.canaries_intact(), f"{N1}x{N2} direction {direction}: the call wrote outside its {name} buffer"
    res = out.mid.cpu()
    if rc == 0 and not raw:
        res = res.reshape(B, 2, KX) if direction == 0 else res.reshape(B, L)
    return res, rc


def run_case(c, K2, B=2):
    """One row of the table, both directions, against the float64 references: dict of the per-row errors and the adjoint gap."""
    N1, N2, rad1, rad2 = c[:4]
    L, KX = N1 * N2, K2 * N1
    x, G = inputs(L, KX, B, seed=1000 + 7 * N1 + N2 + K2)
    Xref, xtref = ref_forward(x, KX), ref_transpose(G, L)
    spec, rc0 = mixed_call(x, N1, N2, K2, rad1, rad2, 0)
    xt, rc1 = mixed_call(G, N1, N2, K2, rad1, rad2, 1)
    assert rc0 == 0 and rc1 == 0, (rc0, rc1)
    gap, gap_bar = adjoint_gap(spec, G, x, xt, Xref, xtref)
    return dict(case=case_id(c), K2=K2, fwd=row_err(as_complex(spec), Xref), tr=row_err(xt.double(), xtref), gap=gap, gap_bar=gap_bar)


def run_front_end(fft, B, seed):
    """RealFFT.rfft over all KX bins and RealFFT.rfft_T, against the same two references."""
    L, KX = fft.L, fft.KX
    x, G = inputs(L, KX, B, seed)
    Xref, xtref = ref_forward(x, KX), ref_transpose(G, L)
    spec = fft.rfft(x.cuda())
    xt = fft.rfft_T(G.cuda())
    torch.cuda.synchronize()
    gap, gap_bar = adjoint_gap(spec, G, x, xt, Xref, xtref)
    return dict(L=L, B=B, fwd=row_err(as_complex(spec), Xref), tr=row_err(xt.double().cpu(), xtref), gap=gap, gap_bar=gap_bar)


def main():
    """Child process of tests/test_gpu_fft.py: the whole table, one JSON line per run."""
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    for c, K2 in runs():
        print("FFT_CASE " + json.dumps(run_case(c, K2)), flush=True)
    print("FFT_CASES_DONE", flush=True)


if __name__ == "__main__":
    main()
