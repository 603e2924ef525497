"""Frequency-resolved error on the GPU: babe_plane_bin_energy (csrc/loss.hip) element by element against the float64 sum of the
same fp32 inputs, and CQT_nsgt.band_energy against the float64 oracle transform.  Needs a MI355X.

The kernel's bound.  Every term re^2 + im^2 is non-negative, so the relative error of a sum is at most the number of roundings
the longest path from an input to the output passes, times 2^-24 (to first order).  The paths: the term (one product, one fused
multiply-add: 2), the thread's serial sum (at most ceil(T / 256) - 1 additions that round; the 16-byte path sums four terms as
a pair of pairs and then ceil(T / 1024) - 1 more), six steps down the wave, two across the four waves, one division: at most
ceil(T / 256) + 11 in all.  At the T of the cases below that is
    T = 1: 12,  3: 12,  64: 12,  262: 13,  260: 13,  4096: 27      (times 2^-24 = 5.96e-8)."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# (B, F, T, offset of the view inside its buffer in floats)
CASES = [(1, 1, 1, 0), (2, 3, 3, 0), (2, 64, 64, 0), (1, 5, 262, 0), (2, 4, 260, 1), (1, 64, 4096, 0)]
ROUNDINGS = {1: 12, 3: 12, 64: 12, 262: 13, 260: 13, 4096: 27}


def nan_framed(B, F, T, off, seed):
    """A contiguous [B,2,F,T] view `off` floats into a NaN-filled device buffer (NaN before and behind it), and its CPU copy."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 2, F, T, generator=g) * torch.logspace(-2, 1, F).reshape(1, 1, F, 1)
    n = x.numel()
    buf = torch.full((n + 64,), float("nan"), device="cuda")
    # the allocation is 16-byte aligned (asserted), so off = 4 k keeps rows with T % 4 == 0 aligned and off = 1 breaks them
    assert buf.data_ptr() % 16 == 0
    start = 32 + off
    buf[start:start + n] = x.reshape(-1).cuda()
    return buf[start:start + n].view(B, 2, F, T), x


@pytest.mark.parametrize("B,F,T,off", CASES)
def test_kernel_vs_float64_sum(B, F, T, off):
    from babe_amd.stft import plane_bin_energy
    assert ROUNDINGS[T] == math.ceil(T / 256) + 11
    c, x = nan_framed(B, F, T, off, seed=T)
    assert c.is_contiguous() and (c.data_ptr() % 16 == 0) == (off % 4 == 0)
    out = torch.full((B * F + 8,), float("nan"), device="cuda")
    o = out[4:4 + B * F].view(B, F)
    plane_bin_energy(c, o)
    o2 = plane_bin_energy(c)
    torch.cuda.synchronize()
    assert torch.equal(o, o2)                                             # two runs agree bit for bit
    assert bool(torch.isnan(out[:4]).all()) and bool(torch.isnan(out[4 + B * F:]).all())      # nothing written outside
    ref = (x.double() ** 2).sum(1).mean(-1)                               # [B,F], float64 sum of the same fp32 inputs
    relerr = ((o.double().cpu() - ref).abs() / ref).max().item()
    bound = ROUNDINGS[T] * 2.0 ** -24
    print(f"(B,F,T)=({B},{F},{T}) off {off}: max relative error {relerr:.3e}, bound {bound:.3e}")
    assert bool(torch.isfinite(o).all())
    assert relerr <= bound


def test_argument_errors_write_nothing():
    from babe_amd._lib import BabeHipError, lib, ptr, stream
    from babe_amd.stft import plane_bin_energy
    c = torch.ones(1, 2, 2, 4, device="cuda")
    out = torch.full((2,), 7.0, device="cuda")
    L = lib()
    for B, F, T in ((0, 2, 4), (1, 0, 4), (1, 2, 0), (-1, 2, 4), (1, -2, 4), (1, 2, -4)):
        assert L.babe_plane_bin_energy(ptr(c), ptr(out), B, F, T, stream()) == -1          # BABE_ERR_ARG
    assert L.babe_plane_bin_energy(None, ptr(out), 1, 2, 4, stream()) == -1
    assert L.babe_plane_bin_energy(ptr(c), None, 1, 2, 4, stream()) == -1
    torch.cuda.synchronize()
    assert out.tolist() == [7.0, 7.0]
    assert b"plane_bin_energy" in L.babe_last_error()
    with pytest.raises(ValueError):
        plane_bin_energy(c[:, :, :, ::2])                                  # not contiguous
    with pytest.raises(ValueError):
        plane_bin_energy(c, torch.empty(1, 3, device="cuda"))              # wrong output shape
    with pytest.raises(RuntimeError):
        plane_bin_energy(torch.ones(1, 2, 2, 4))                           # no CPU path
    assert BabeHipError is not None


FS, L = 22050, 92092


@pytest.fixture(scope="module")
def cqt():
    from babe_amd.cqt import CQT_nsgt
    return CQT_nsgt(7, 64, "oct", ("kaiser", 1), FS, L, device="cuda")


def test_band_energy_vs_oracle_float64(cqt):
    """Bar: tests/test_gpu_cqt.py holds the forward coefficients to 2e-5 of the octave's largest; energy is quadratic in the
    coefficients, so its relative error is twice theirs to first order: ||a - b|| / ||b|| < 4e-5 per row."""
    from oracle.nsgt import CQT_nsgt as OracleCQT
    g = torch.Generator().manual_seed(2)
    x = 0.1 * torch.randn(2, L, generator=g)
    got = cqt.band_energy(x.cuda())
    got2 = cqt.band_energy(x.cuda())
    assert got.shape == (2, 7 * 64) and torch.equal(got, got2)
    orc = OracleCQT(7, 64, "oct", ("kaiser", 1), FS, L, dtype=torch.float64)
    ref = torch.cat([c.squeeze(1).abs().pow(2).mean(-1) for c in orc.fwd(x.double().unsqueeze(1))], dim=1)      # [B, 448]
    for b in range(2):
        rel = float((got[b].double().cpu() - ref[b]).norm() / ref[b].norm())
        print(f"row {b}: ||a-b||/||b|| = {rel:.3e}")
        assert rel < 2 * 2e-5


@pytest.mark.parametrize("k", [5, 200, 300, 440])
def test_sine_at_a_bin_centre_peaks_in_that_bin(cqt, k):
    f = float(cqt.design["f"][k])
    t = torch.arange(L, dtype=torch.float64) / FS
    x = (0.1 * torch.sin(2 * np.pi * f * t)).float().reshape(1, L)
    e = cqt.band_energy(x.cuda())[0]
    assert int(e.argmax()) == k, (k, int(e.argmax()))
