"""What the HuBERT tests and tests/golden/make_golden_hubert.py share: the golden cases with their configs, synthetic weights and waveforms,
the sub-sampling of the stored taps and the tolerance.  Imported by tests; it holds none."""
import functools

import numpy as np
import torch

from conftest import load_golden
from real3dportrait_amd import synth

TOL = 2e-4          # of max|ref|
QK_GAIN = 2.0
SMALL = {"hidden_size": 128, "num_hidden_layers": 2, "num_attention_heads": 2, "intermediate_size": 256, "conv_dim": (32,) * 7,
         "num_conv_pos_embeddings": 16, "num_conv_pos_embedding_groups": 4}
WIDE = {"num_hidden_layers": 1}          # the product widths of synth.HUBERT_LARGE, one layer
CONFIGS = {"small": SMALL, "wide": WIDE}
# name -> (config, samples, weight seed, waveform seed, row step of the stored taps); tests/golden/<name>.npz
CASES = {"hubert_a_n330123": ("small", 330123, 81, 82, 8),
         "hubert_b_n4077": ("small", 4077, 81, 83, 1),
         "hubert_c_wide_n12000": ("wide", 12000, 84, 85, 2)}
TAPS = ("extract_features", "projected", "pos_conv", "layer0")


def config(name):
    """The full width set of a config name: synth.HUBERT_LARGE with the case's overrides."""
    return dict(synth.HUBERT_LARGE, **CONFIGS[name])


def waveform(seed, n):
    """A speech-like clip as sf.read returns it (float64, PCM-16 values): an amplitude-modulated 220 Hz tone (a parabolic sine, so that no
    libm call decides a bit), noise and a DC offset, quantised to int16 / 32768."""
    i = np.arange(n, dtype=np.int64)
    para = lambda f_num, f_den: (lambda u: 4.0 * u * (1.0 - np.abs(u)))(2.0 * ((i * f_num) % f_den).astype(np.float64) / f_den - 1.0)
    tone = 0.3 * (0.6 + 0.4 * para(3, 16000)) * para(220, 16000)
    x = tone + 0.05 * synth.hash_unitvar(seed, (n,), stream=8).astype(np.float64) + 0.02
    return np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16).astype(np.float64) / 32768.0


@functools.lru_cache(maxsize=4)
def weights(seed, cfg_name):
    """synth.synth_hubert as torch tensors (cached)."""
    return {k: torch.from_numpy(v) for k, v in synth.synth_hubert(seed, CONFIGS[cfg_name], qk_gain=QK_GAIN).items()}


def case_inputs(name):
    """(config name, full config, state_dict, waveform float64 numpy [n])."""
    cfg_name, n, seed_w, seed_x, _ = CASES[name]
    return cfg_name, config(cfg_name), weights(seed_w, cfg_name), waveform(seed_x, n)


def golden_case(name):
    return (load_golden(name),) + case_inputs(name)


def tap_rows(name, t):
    """The stored part of a tap [T, C] of the first chunk."""
    return t[::CASES[name][4]]


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


def hip_model(cfg_name, sd, dev):
    from real3dportrait_amd.hubert import HubertFeatureModel
    m = HubertFeatureModel(CONFIGS[cfg_name])
    m.load_state_dict(sd, strict=True)
    return m.to(dev).eval()
