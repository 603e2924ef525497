"""Seeded weights of the frequency-encoding goldens (tests/golden/make_fencoding_golden.py, which imports the reference, and the
GPU tests, which must not): only outputs are stored in the fixtures, the weights are re-derived here from seeds."""
from tests.attention_weights import LAST_TWO, SMALL_DILS, SMALL_NS, attention_dict, scale_attention
from tests.golden_weights import scale_gates

FS, L = 22050, 92092
# fixture name -> (attention_layers, attention_dict, batch)
FIXTURES = {
    "a": (None, None, 2),                          # encodings only: forward, input-VJP and every parameter gradient
    "b": (LAST_TWO, attention_dict(), 1),          # encodings + time attention: forward and input-VJP
}


def fencoding_sd(name, seed=0):
    """babe_amd's init_state_dict(seed, use_fencoding=True) with O(1) gates, then scale_gates (and scale_attention)."""
    from babe_amd.networks.cqtdiff_plus import init_state_dict
    layers, adict, _ = FIXTURES[name]
    sd = init_state_dict(SMALL_NS, SMALL_DILS, seed=seed, gate_scale=1.0, attention_layers=layers, attention_dict=adict,
                         use_fencoding=True)
    sd = scale_gates(sd, seed=5)
    return scale_attention(sd) if layers else sd
