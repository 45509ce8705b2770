"""What the img2plane tests and tests/golden/make_golden_img2plane.py share: the stand-in for DeepLabV3, the golden cases with their inputs and
synthetic weights, and a plain-torch stand-in of the reference's Img2PlaneModel for the patch_model tests.  Imported by tests; it holds none."""
import functools

import numpy as np
import torch
import torch.nn as nn

import img2plane_ref64 as R64
from conftest import load_golden
from real3dportrait_amd import synth

TOL = 2e-4          # of max|ref|
QK_GAIN = 1.5
MODE_CHANNELS = {"rgb": 3, "rgb_alpha": 4, "rgb_camera": 6, "rgb_alpha_camera": 7}
# name -> (mode, scale, S, B, weight seed, input seed); tests/golden/<name>.npz
CASES = {"img2plane_a_s64_b2": ("rgb", "standard", 64, 2, 71, 72),
         "img2plane_b_s96": ("rgb", "small", 96, 1, 73, 74),
         "img2plane_c_s80_alpha": ("rgb_alpha", "small", 80, 1, 75, 76)}
TAPS = ("feat_low", "feat_low_after_vit", "feat_high", "predictor_tokens")
# how each tap is sub-sampled in the golden files (the planes are whole): a slice per tap, applied to [B, C, H, W]
TAP_SLICES = {"feat_low": np.s_[:, ::8], "feat_low_after_vit": np.s_[:, ::8, ::2, ::2], "feat_high": np.s_[:, ::8, ::2, ::2],
              "predictor_tokens": np.s_[:, ::128]}


class StandInEncoder(nn.Module):
    """In the place of DeepLabV3(in_channels): [B, C, S, S] -> [B, 256, S/8, S/8], an 8 x 8 average pool and a 1 x 1 conv whose weights
    come from the seed.  Deterministic, torch only; the golden maker and the tests use this one."""

    def __init__(self, in_channels, seed=70):
        super().__init__()
        self.pool = nn.AvgPool2d(8)
        self.proj = nn.Conv2d(in_channels, 256, 1)
        w = synth.hash_unitvar(seed, (256, in_channels, 1, 1), stream=4900) * np.float32(3.0 / np.sqrt(in_channels))
        b = synth.hash_unitvar(seed, (256,), stream=4901) * np.float32(0.5)
        with torch.no_grad():
            self.proj.weight.copy_(torch.from_numpy(w))
            self.proj.bias.copy_(torch.from_numpy(b))

    def forward(self, x):
        return self.proj(self.pool(x))


def image(seed, B, S, black_rows=0):
    """A portrait-like image in [-1, 1]: 8 x 8 blocks of one value each plus pixel noise; the first `black_rows` rows are exactly -1 in
    every channel (the background the rgb_alpha modes mask, img2plane_model.py:49)."""
    coarse = synth.hash_uniform(seed, B * 3 * (S // 8) ** 2, stream=5).reshape(B, 3, S // 8, S // 8) * np.float32(2.0) - np.float32(1.0)
    fine = synth.hash_uniform(seed, B * 3 * S * S, stream=6).reshape(B, 3, S, S) * np.float32(2.0) - np.float32(1.0)
    x = np.float32(0.7) * np.repeat(np.repeat(coarse, 8, axis=2), 8, axis=3) + np.float32(0.3) * fine
    x[:, :, :black_rows] = np.float32(-1.0)
    return np.ascontiguousarray(x, dtype=np.float32)


@functools.lru_cache(maxsize=4)
def weights(seed, scale, in_channels):
    """synth.synth_img2plane as torch tensors (cached: the standard scale is 57 M parameters)."""
    return {k: torch.from_numpy(v) for k, v in synth.synth_img2plane(seed, scale, in_channels, qk_gain=QK_GAIN).items()}


def case_inputs(name):
    """(mode, scale, in_channels, state_dict without the encoder's keys, image [B, 3, S, S] float32 numpy)."""
    mode, scale, S, B, seed_w, seed_x = CASES[name]
    cin = MODE_CHANNELS[mode] + 2
    return mode, scale, cin, weights(seed_w, scale, cin), image(seed_x, B, S, black_rows=S // 4 if "alpha" in mode else 0)


def golden_case(name):
    return (load_golden(name),) + case_inputs(name)


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


def hip_model(mode, scale, sd, dev, out_channels=96):
    """The package's module with the stand-in encoder, weights loaded from a state_dict that lacks the encoder's keys."""
    from real3dportrait_amd.img2plane import Img2PlaneModel
    m = Img2PlaneModel(out_channels, hp={"img2plane_input_mode": mode, "img2plane_backbone_scale": scale},
                       low_reso_encoder=StandInEncoder(MODE_CHANNELS[mode] + 2))
    full = dict(sd)
    full.update({"low_reso_encoder." + k: v for k, v in m.low_reso_encoder.state_dict().items()})
    m.load_state_dict(full, strict=True)
    return m.to(dev).eval()


class _Holder(nn.Module):
    pass


class Img2PlaneModel(nn.Module):
    """A plain-torch stand-in with the reference's class name, attribute names and state_dict keys (what patch_model looks at), computing
    through tests/img2plane_ref64.py in float32."""

    def __init__(self, mode="rgb", scale="small", out_channels=96):
        super().__init__()
        self.hparams = {"img2plane_input_mode": mode, "img2plane_backbone_scale": scale}
        self.input_mode = mode
        cin = MODE_CHANNELS[mode] + 2
        self.low_reso_encoder = StandInEncoder(cin)
        for key, shape in synth.img2plane_shapes(scale, cin, out_channels):
            owner, parts = self, key.split(".")
            for p in parts[:-1]:
                if not hasattr(owner, p):
                    setattr(owner, p, _Holder())
                owner = getattr(owner, p)
            setattr(owner, parts[-1], nn.Parameter(torch.zeros(shape)))
        self.low_reso_vit.num_blocks, self.triplane_predictor_vit.num_blocks = synth.IMG2PLANE_BLOCKS[scale]
        self.triplane_predictor_vit.final_conv.out_channels = out_channels

    @torch.no_grad()
    def forward(self, x, cond=None, **kw):
        from real3dportrait_amd.img2plane import Img2PlaneModel as Hip
        x_in = Hip.assemble_input(self, x, cond)
        return R64.forward(self.state_dict(), x_in, self.low_reso_encoder(x_in), torch.float32)[0]
