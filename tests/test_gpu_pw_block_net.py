"""The fused (1,1) ResnetBlock passes (csrc/pw_block.hip) inside the full-width network, at the octave lengths Ts = 16 * 2^j of
tests/test_gpu_unet_c.py: switch on against switch off (the same numbers added in another order: 2e-5 of the maximum, the bar the
project uses for that), and the Python sequencer against the library-side one under the switch (same entry points, so the same
bits and the same launches)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

NS, ND = [64, 96, 96, 128, 128, 256, 256], [2, 3, 4, 5, 6, 7, 7]


@pytest.fixture(scope="module")
def sd():
    from babe_amd.networks.cqtdiff_plus import init_state_dict
    return {k: v.cuda() for k, v in init_state_dict(NS, ND, seed=3, gate_scale=1.0).items()}


@pytest.fixture
def switch():
    """Sets the library's switch for the test and restores what the process had."""
    from babe_amd import ops
    prev = ops.pw_block_enable(True)
    try:
        yield ops.pw_block_enable
    finally:
        ops.pw_block_enable(prev)


def _run(sd, unet_c, C_list, gouts, cn, monkeypatch):
    from babe_amd._lib import dispatch_counts
    from babe_amd.forms import FORMS
    from babe_amd.networks import unet_engine as ue
    monkeypatch.setattr(FORMS, "unet_c", unet_c)
    eng = ue.UnetEngine(sd, NS, ND)
    assert (eng._c_engine() is not None) == unet_c
    film = eng.embed(cn)
    dispatch_counts(reset=True)
    outs = eng.forward(C_list, film)
    gC = eng.vjp(gouts)
    torch.cuda.synchronize()
    return [t.clone() for t in outs + gC], dispatch_counts()


@pytest.mark.parametrize("B", [1, 2])
def test_network_with_and_without_the_fused_blocks(sd, switch, monkeypatch, B):
    gen = torch.Generator().manual_seed(20 + B)
    C_list = [torch.randn(B, 2, 64, 16 * 2 ** j, generator=gen).cuda() for j in range(7)]
    gouts = [torch.randn(c.shape, generator=gen).cuda() for c in C_list]
    cn = torch.linspace(-1.1, -0.4, B).reshape(B, 1).cuda()
    switch(False)
    off, n_off = _run(sd, False, C_list, gouts, cn, monkeypatch)
    switch(True)
    on, n_on = _run(sd, False, C_list, gouts, cn, monkeypatch)
    on_c, n_on_c = _run(sd, True, C_list, gouts, cn, monkeypatch)
    print(f"B={B}: conv11 launches off {n_off['conv11']} on {n_on['conv11']}; all launches off {sum(n_off.values())} on {sum(n_on.values())}")
    assert n_on["conv11"] < n_off["conv11"], (n_on["conv11"], n_off["conv11"])
    for a, b in zip(on, off):
        d = float((a - b).abs().max() / b.abs().max())
        print(f"  on vs off: {d:.2e}")
        assert d <= 2e-5, d
    for a, b in zip(on, on_c):
        assert torch.equal(a, b)
    # The same launches - except that for B > 1 the library-side sequencer makes every layer's gate rows contiguous with
    # babe_axpby4d, where the Python one uses a torch copy: one 'axpby' launch per dilation layer, whatever the switch.
    layers = 2 * sum(ND) + ND[-1] + 2 * len(NS) + 1           # main + up blocks, the middle block, init blocks + heads, mid_out
    want = dict(n_on, axpby=n_on["axpby"] + (layers if B > 1 else 0))
    assert n_on_c == want, {k: (want[k], n_on_c[k]) for k in want if want[k] != n_on_c[k]}
