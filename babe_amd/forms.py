"""The A/B switches of the UNet layer path (ops.py, networks/unet_engine.py, csrc/unet_engine.hip), declared once.

Every switch chooses between bit-identical or parity-checked forms of the same layer.  TABLE is the list: attribute of FORMS,
environment variable, default, parsing rule, what the non-default value selects.  ops.py and unet_engine.py read FORMS.<name>
where they act on it and keep no copy; a test selects a form with monkeypatch.setattr(FORMS, name, value), which undoes itself.

Two of them, fuse_gn_fwd and fuse_gn, are acted on by BOTH sequencers, so the library owns them: it alone reads their
environment variables, and FORMS.fuse_gn_fwd / FORMS.fuse_gn are views of babe_unet_form_get / babe_unet_form_set - read from
the library on first use, cached here (no C call per launch), written through on assignment.  Their rules below say what the
library does (tests/test_forms_cpu.py compares), and are never applied to the environment by this module.
"""
import os
import re


def _unless_0(v):
    return v != "0"


def _only_1(v):
    return v == "1"


def _atoi(v):
    """C's atoi: the leading integer of the string, 0 if there is none."""
    m = re.match(r"\s*[+-]?\d+", v)
    return int(m.group()) if m else 0


# (attribute, environment variable, default, rule: string -> value, what the non-default value selects)
TABLE = (
    ("bf16_hbm_f32", "BABE_BF16_HBM_F32", "1", _unless_0,
     "0: under 'bf16' / 'bf16x3' the few-channel and HBM-bound (1,1) convs take the bf16 kernels too instead of the fp32 ones"),
    # debug switch for the (5,3) fp32 convs: 0 = direct kernel only, 2 = Winograd F(2,3) only, 4 (default) = F(4,3) where the
    # problem qualifies, F(2,3) otherwise
    ("conv_wino", "BABE_CONV_WINO", "4", str,
     "'0': direct kernels only; '1' or '2': Winograd F(2,3) only (no F(4,3), no nested kernel); anything else: F(4,3) too"),
    ("fewco", "BABE_CONV_FEWCO", "1", _unless_0,
     "0: no raw-weight image, so the few-output-channel kernel never runs"),
    # nested Winograd F(2,5) x F(4,3) (csrc/conv_wino45.hip) for the (5,3) layers it supports.  Read by the library as well
    # (babe_conv2d_wino45_supported refuses at 0): either side being off is enough, so the two cannot contradict each other
    ("wino45", "BABE_CONV_WINO45", "1", _unless_0,
     "0: the F(4,3) kernels instead of the nested F(2,5) x F(4,3) ones; also switches the F(4,5) kernel off"),
    # nested Winograd F(4,5) x F(4,3) (csrc/conv_wino85.hip) for the (5,3) layers with 128-channel output tiles whose row quads
    # are at least 80 % full (the rule babe_conv2d_auto applies)
    ("f45", "BABE_CONV_F45", "1", _unless_0,
     "0: no F(4,5) x F(4,3) images: those layers are left to the F(2,5) x F(4,3) kernel"),
    # (1,1) convs: 64-channel output tiles per workgroup (two 32-row tiles) wherever both directions' tile counts are even, instead
    # of the library default of up to 128: more workgroups on the small planes of the deep levels, where a launch has a few hundred
    # (whole-job A/B, same box: 2.431 / 2.432 vs 2.423 / 2.424 audio-sec/s; one tile: 2.399 / 2.395)
    ("conv11_nt", "BABE_CONV11_NT", "2", int,
     "row tiles (x32 output channels) per workgroup of the (1,1) convs; 0: the library default"),
    # GroupNorm-VJP partial sums formed in the F(4,5) transposed conv's epilogue instead of babe_gn_bwd_partial's own pass: OFF by
    # default - measured 0.5 % slower than the separate pass (profiles/r06_gn_fusion_experiment.txt: the GELU' arithmetic runs on
    # the multiply waves with nothing to overlap it); tests/test_gpu_ops.py keeps it parity-checked.  Owned by the library
    ("fuse_gn", "BABE_FUSE_GN", "0", lambda v: _atoi(v) != 0,
     "a non-zero number: the GroupNorm-VJP sums come out of the transposed F(4,5) conv's epilogue (stat_mode 2)"),
    # The NEXT layer's GroupNorm sums (sum, sum of squares of the output) formed in the forward F(4,5) conv's epilogue instead of
    # babe_gn_partial's pass over the freshly written output: two double additions per output, no extra loads.  Owned by the library
    ("fuse_gn_fwd", "BABE_FUSE_GN_FWD", "1", lambda v: _atoi(v) != 0,
     "0: the next layer's GroupNorm sums in babe_gn_partial's own pass instead of the conv's epilogue (stat_mode 1)"),
    # Measured (round 4, same box, A/B/A/B): the one-launch form is SLOWER on the whole job - 1.992 / 1.991 vs 2.080 / 2.079
    # audio-sec/s - every workgroup of a 10 us streaming kernel pays a device-scope fence + an atomic before it retires, and the
    # last one a serial tail; the separate 3.5 us finalize launch overlaps the other lane's kernels instead
    ("gn_fused", "BABE_GN_FUSED", "0", _only_1,
     "1: GroupNorm statistics in one launch (the last workgroup of a group finalises it) instead of partial sums + finalize"),
    ("gelu_fin", "BABE_GELU_FIN", "1", _unless_0,
     "0: gn_scale followed by scale_gelu instead of the finalize folded into the GELU kernel's prologue"),
    # Read by the library as well (babe_conv2d_bf16_units_supported refuses at 0): either side off is enough, as for wino45
    ("units", "BABE_CONV_BF16U", "1", _unless_0,
     "0: the bf16 (5,3) forward convs read fp32 activations instead of bf16 units"),
    ("axpby2", "BABE_AXPBY2", "1", _unless_0,
     "0: the two-pass forms of the merged element-wise passes"),
    # the library-side sequencer (csrc/unet_engine.hip): one C call per direction (fp32 networks without attention)
    ("unet_c", "BABE_UNET_C", "0", _only_1,
     "1: UnetEngine runs forward and input-VJP on the library-side sequencer"),
    ("merge_tail", "BABE_MERGE_TAIL", "1", _unless_0,
     "0: the N -> N block VJP stores gz and merges with axpby2 instead of merging in the last layer's pass"),
)

LIBRARY_OWNED = ("fuse_gn_fwd", "fuse_gn")          # index = which of babe_unet_form_get / babe_unet_form_set


def parse(environ):
    """{attribute: value} of every switch of TABLE under the environment mapping `environ`."""
    return {name: rule(environ.get(var, default)) for name, var, default, rule, _ in TABLE}


def _library_form(which):
    def get(self):
        if self._lib[which] is None:
            from ._lib import lib
            self._lib[which] = bool(lib().babe_unet_form_get(which))
        return self._lib[which]

    def put(self, on):
        from ._lib import check, lib
        check(lib().babe_unet_form_set(which, int(bool(on))), "unet_form_set")
        self._lib[which] = bool(on)

    return property(get, put)


class Forms:
    """The values: plain attributes, the Winograd families derived from the three stored ones, the two library-owned views."""

    def __init__(self, environ):
        self._lib = [None, None]                    # the library's two values as last read or written here
        for name, value in parse(environ).items():
            if name not in LIBRARY_OWNED:
                setattr(self, name, value)

    winograd = property(lambda self: self.conv_wino != "0")                     # F(2,3) along time
    winograd4 = property(lambda self: self.conv_wino not in ("0", "2", "1"))    # F(4,3) along time
    winograd45 = property(lambda self: self.winograd4 and self.wino45)          # nested F(2,5) x F(4,3)
    winograd85 = property(lambda self: self.winograd45 and self.f45)            # nested F(4,5) x F(4,3)
    fuse_gn_fwd = _library_form(0)
    fuse_gn = _library_form(1)


FORMS = Forms(os.environ)
