"""Plain-YAML config loader producing the attribute-style nested mapping the reference reads
(OmegaConf in the reference: test.py:69).  PyYAML parses exponent floats without a dot
('1e-4') as strings; they are coerced to float like OmegaConf does."""
import re

_FLOAT = re.compile(r"[+-]?(\d+\.?\d*|\.\d+)[eE][+-]?\d+")


class AttrDict(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e

    def __setattr__(self, k, v):
        self[k] = v


def to_attr(o):
    if isinstance(o, dict):
        return AttrDict({k: to_attr(v) for k, v in o.items()})
    if isinstance(o, (list, tuple)):
        return [to_attr(v) for v in o]
    if isinstance(o, str) and _FLOAT.fullmatch(o):
        return float(o)
    return o


def load_yaml(path):
    import yaml
    with open(path) as f:
        return to_attr(yaml.safe_load(f))


def parse_value(text):
    """The value of a `key.sub=value` override, read as YAML reads a scalar or a flow list ('3', '2e-4', 'True', '[1, 2]',
    'None' stays the string the reference's configurations use), with load_yaml's float coercion."""
    import yaml
    return to_attr(yaml.safe_load(text))


def apply_overrides(args, overrides):
    """Apply ['exp.lr=1e-4', 'dset.years=[2017, 2018]', ...] to a nested AttrDict in place; a missing section is created, a
    path through a non-mapping is an error.  Returns args."""
    for item in overrides:
        if "=" not in item:
            raise ValueError(f"override {item!r} is not of the form key.sub=value")
        path, text = item.split("=", 1)
        keys = path.strip().split(".")
        node = args
        for k in keys[:-1]:
            if k not in node:
                node[k] = AttrDict()
            node = node[k]
            if not isinstance(node, dict):
                raise ValueError(f"override {item!r}: {k!r} is not a section")
        node[keys[-1]] = parse_value(text)
    return args


def default_train_args(**kw):
    """default_args(**kw) plus what training reads: the training keys of conf/exp/maestro44k_8s.yaml, conf/dset/maestro_allyears.yaml
    as `dset`, and a `logging` section (values restated; tests/test_train_conf_cpu.py holds them against the files).
    Carried but never read, by the reference's loop or by ours: exp.scheduler_step_size / scheduler_gamma (no scheduler is ever
    built), exp.use_fp16 (precision is the network's and set_trainable's), exp.augmentations (marked TODO there, never applied).
    exp.model_dir is where checkpoints and the log go; the reference reads a top-level model_dir (conf/conf.yaml), which is set
    to the same value.  The reference ships no conf/logging file; the logging values are this tree's choice and only the keys
    the reference's trainer reads are kept (log, log_interval, save_model, save_interval, remove_last_checkpoint,
    num_sigma_bins, freq_cqt_logging)."""
    a = default_args(**kw)
    a.exp.update(to_attr(dict(
        exp_name="44k_8s", model_dir="None",
        optimizer=dict(type="adam", beta1=0.9, beta2=0.999, eps=1e-8),
        lr=2e-4, lr_rampup_it=10000, scheduler_step_size=60000, scheduler_gamma=0.8,
        batch=4, num_accumulation_rounds=1, use_fp16=False, num_workers=4,
        seed=42, resume=True, resume_checkpoint="None", resample_factor=1,
        ema_rate=0.9999, ema_rampup=10000, use_grad_clip=True, max_grad_norm=1,
        augmentations=dict(rev_polarity=True, pitch_shift=dict(use=False, min_semitones=-6, max_semitones=6),
                           gain=dict(use=False, min_db=-3, max_db=3)))))
    a.model_dir = a.exp.model_dir
    a.dset = to_attr(dict(
        name="maestro_allyears", callable="datasets.maestro_dataset.MaestroDataset_fs", type="audio",
        path="/scratch/shareddata/dldata/maestro/v3.0.0/maestro-v3.0.0",
        years=[2004, 2006, 2008, 2009, 2011, 2013, 2014, 2015, 2017, 2018], years_test=[2009], cache=True, load_len=405000))
    a.logging = to_attr(dict(log=True, log_interval=1, save_model=True, save_interval=50000, remove_last_checkpoint=False,
                             num_sigma_bins=20, freq_cqt_logging=50))
    return a


def default_args(sample_rate=44100, audio_len=368368, Ns=(64, 96, 96, 128, 128, 256, 256), T=35, xi=0.2,
                 start_sigma=0.2):
    """The blind-BWE configuration the benchmark is quoted on: conf/tester/blind_bwe_formal_3000_opt_2.yaml,
    conf/network/cqtdiff+.yaml, conf/exp/maestro44k_8s.yaml, conf/diff_params/edm.yaml (values restated)."""
    return to_attr(dict(
        exp=dict(sample_rate=sample_rate, audio_len=audio_len),
        network=dict(use_fencoding=False, use_norm=True, emb_dim=256, Ns=list(Ns), Ss=[2] * 7,
                     num_dils=[2, 3, 4, 5, 6, 7, 7], attention_layers=[0] * 8, attention_dict=None,
                     bottleneck_type="res_dil_convs", num_bottleneck_layers=1,
                     cqt=dict(window="kaiser", beta=1, num_octs=7, bins_per_oct=64)),
        diff_params=dict(sigma_data=0.063, sigma_min=1e-5, sigma_max=10, P_mean=-1.2, P_std=1.2, ro=13, ro_train=10,
                         Schurn=5, Snoise=1, Stmin=0, Stmax=50, aweighting=dict(use_aweighting=False, ntaps=101)),
        tester=dict(
            T=T, order=2, filter_out_cqt_DC_Nyq=True,
            posterior_sampling=dict(xi=xi, data_consistency=False, norm=2, smoothl1_beta=1, SNR_observations="None",
                                    start_sigma=start_sigma, freq_weighting="None", freq_weighting_filter="sqrt",
                                    stft_distance=dict(mag=False, logmag=False, use=False, use_multires=False, nfft=2048)),
            diff_params=dict(same_as_training=False, sigma_data=0.063, sigma_min=1e-4, sigma_max=1, ro=8, Schurn=10,
                             Snoise=1.0, Stmin=0, Stmax=50),
            blind_bwe=dict(NFFT=4096, fcmin=20, fcmax="nyquist", Amin=-50, Amax=30, sigma_den_estimate=0.0,
                           SNR_observations="None",
                           initial_conditions=dict(fc=[280, 285, 290, 295, 300], A=[-15, -17, -20, -25, -30]),
                           optimization=dict(max_iter=100, tol=[5e-3, 5e-3], mu=[1000, 10], clamp_fc=True,
                                             clamp_A=True, only_negative_A=True)),
            complete_recording=dict(inpaint_DC=True))))
