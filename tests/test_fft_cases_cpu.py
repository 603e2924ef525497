"""The float64 references and the case table of tests/test_gpu_fft.py, pinned without a GPU: the table's radix lists and the
passes they reach, the explicit matrix of the forward map against the two FFT-based references, and the factorisations RealFFT
picks for the lengths the GPU tests send through it."""
import numpy as np
import pytest
import torch

from tests import fft_cases as fc

SMALL = [(c, K2) for c, K2 in fc.runs() if c[0] * c[1] <= 2112]
# RealFFT lengths of the GPU tests: (L, N1, N2, rad1, rad2); None = outside the radix set (dense fallback)
FRONT_END = [(6, 2, 3, [2], [3]), (35, 5, 7, [5], [7]), (210, 14, 15, [2, 7], [3, 5]), (2002, 26, 77, [2, 13], [7, 11]),
             (2112, 44, 48, [4, 11], [4, 4, 3]), (13860, 110, 126, [2, 5, 11], [2, 3, 3, 7]),
             (323, 17, 19, None, None), (1798, 31, 58, None, None)]


def test_radix_lists_multiply_to_their_factor_and_are_admitted():
    for N1, N2, rad1, rad2, _, _ in fc.CASES:
        for N, rad in ((N1, rad1), (N2, rad2)):
            assert int(np.prod(rad)) == N and 1 <= len(rad) <= 6 and set(rad) <= set(fc.RADICES), (N, rad)
            assert (2 * N * 7 + N) * 8 <= 160 * 1024, f"N = {N} needs more LDS than the kernel may ask for"
    assert (2 * 1366 * 7 + 1366) * 8 > 160 * 1024                       # 1365 is the largest N of any kind
    assert len({fc.case_id(c) for c in fc.CASES}) == len(fc.CASES)


def test_every_radix_is_a_first_pass_and_a_later_pass_somewhere():
    first, later = fc.pass_positions()
    assert first == set(fc.RADICES) and later == set(fc.RADICES), (sorted(first), sorted(later))


def test_the_table_reaches_what_it_says():
    by = {fc.case_id(c): c for c in fc.CASES}
    tiles = lambda n: -(-n // 14)                                         # packed stage-1 tiles of 14 real columns
    assert tiles(3) == 1 and by["2x3"][1] < 7
    assert (5 * 7) % 2 == 1
    assert by["23x11"][0] > by["23x11"][1]
    assert by["15x14"][1] == 14 and by["14x15"][1] == 14 + 1
    assert by["12x35"][1] == 2 * 14 + 7 and by["12x35"][0] // 2 + 1 == 7
    assert tiles(462) == 33 and -(-(450 // 2 + 1) // 7) == 33
    assert len(by["2x810"][3]) == 6
    assert (2 * 1056 * 7 + 1056) * 8 == 126720 and (2 * 1365 * 7 + 1365) * 8 == 163800
    for c, K2 in fc.runs():
        assert 1 <= K2 <= c[1] and K2 * c[0] > (c[0] * c[1]) // 2          # the half spectrum fits: k <= L/2 < KX
    assert sum(1 for c, K2 in fc.runs() if K2 == c[1] and K2 != fc.k2_of(c[0], c[1])) == 3


@pytest.mark.parametrize("c,K2", SMALL, ids=[f"{fc.case_id(c)}-K2={K2}" for c, K2 in SMALL])
def test_matrix_of_the_forward_map_agrees_with_both_references(c, K2):
    N1, N2 = c[:2]
    L, KX = N1 * N2, K2 * N1
    x, G = fc.inputs(L, KX, 2, seed=5 + L)
    assert bool((G[:, :, L // 2 + 1:] == 0).all()) and bool((G[:, :, : L // 2 + 1] != 0).all())
    M = fc.forward_matrix(L, KX)
    fwd = (x.double() @ M).reshape(2, 2, KX)
    Xref = fc.planar(fc.ref_forward(x, KX))
    assert float((fwd - Xref).abs().max() / Xref.abs().max()) < 1e-12
    tr = G.double().reshape(2, 2 * KX) @ M.T
    xtref = fc.ref_transpose(G, L)
    assert float((tr - xtref).abs().max() / xtref.abs().max()) < 1e-12
    # and the metric sees a one-bin error of the size of the bar in either direction
    bad = fc.ref_forward(x, KX).clone()
    bad[1, KX - 1] += 2 * fc.BAR * Xref[1].abs().max()
    e = fc.row_err(bad, fc.ref_forward(x, KX))
    assert e[0] == 0.0 and e[1] > fc.BAR
    assert np.isnan(fc.row_err(torch.full_like(xtref, float("nan")), xtref)[0])


@pytest.mark.parametrize("L,N1,N2,rad1,rad2", FRONT_END, ids=[str(f[0]) for f in FRONT_END])
def test_factorisations_of_the_front_end_lengths(L, N1, N2, rad1, rad2):
    from babe_amd.cqt import factor_len, small_radices
    assert factor_len(L) == (N1, N2)
    assert small_radices(N1) == rad1 and small_radices(N2) == rad2
