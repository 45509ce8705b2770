"""What the Plane2GridModule tests and tests/golden/make_golden_plane2grid.py share: the golden cases with their inputs and synthetic
weights, the gate, and a plain-torch mock with the reference's class name and attribute layout.  Imported by tests; it holds none."""
import functools

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from real3dportrait_amd import synth

TOL = 2e-4          # of max|branch| = max|y_ref - x|, and of max|tap| for conv1's output
STATS_TOL = 1e-5    # of max(|scale|, |shift|): the statistics entry point against fp64
C, GROUPS = 32, 4
# name -> (N, D, H, W, alpha of each layer, weight seed, input seed); tests/golden/<name>.npz
CASES = {"plane2grid_a_d3_16": (1, 3, 16, 16, (0.37,), 201, 202),
         "plane2grid_b_n2_5x7": (2, 3, 5, 7, (-1.5,), 203, 204),          # 105 rows a sample: every tile straddles samples, M is ragged
         "plane2grid_c_d1_4": (1, 1, 4, 4, (0.8,), 205, 206),             # all three depth taps hit one slice
         "plane2grid_d_d2_9x6": (1, 2, 9, 6, (-0.6,), 207, 208),
         "plane2grid_e_d4_8x12": (1, 4, 8, 12, (0.9, -0.7), 209, 210)}    # depth above 3: two layers


def layers_for(D):
    return 1 if D <= 3 else 2


def state_keys(D):
    """The reference's state_dict keys in its order (SameBlock3d registers conv1, conv2, norm1, norm2 as modules and alpha as a parameter:
    parameters of the block itself come first)."""
    keys = []
    for i in range(layers_for(D)):
        p = "res_blocks_3d.%d." % i
        keys += [p + "alpha"] + [p + m + s for m in ("conv1", "conv2", "norm1", "norm2") for s in (".weight", ".bias")]
    return keys


@functools.lru_cache(maxsize=8)
def weights(seed, D, alphas):
    """Synthetic state_dict: conv weights at 1.4 / sqrt(fan-in), small biases, gamma = 1 + 0.3 g, beta = 0.3 g, alpha away from 0.01."""
    sd = {}
    for i in range(layers_for(D)):
        p, s0 = "res_blocks_3d.%d." % i, 20 * i
        sd[p + "alpha"] = np.array([alphas[i]], np.float32)
        for j, conv in enumerate(("conv1", "conv2")):
            sd[p + conv + ".weight"] = synth.hash_unitvar(seed, (C, C, 3, 3, 3), stream=s0 + 2 * j) * np.float32(1.4 / (27 * C) ** 0.5)
            sd[p + conv + ".bias"] = synth.hash_unitvar(seed, (C,), stream=s0 + 2 * j + 1) * np.float32(0.1)
        for j, norm in enumerate(("norm1", "norm2")):
            sd[p + norm + ".weight"] = np.float32(1.0) + np.float32(0.3) * synth.hash_unitvar(seed, (C,), stream=s0 + 8 + 2 * j)
            sd[p + norm + ".bias"] = np.float32(0.3) * synth.hash_unitvar(seed, (C,), stream=s0 + 9 + 2 * j)
    return {k: torch.from_numpy(np.ascontiguousarray(v, np.float32)) for k, v in sd.items()}


def planes(seed, N, D, H, W):
    """[N, 3 C D, H, W] float32: volume b (of the 3N) is unit-variance noise times (0.5 + 0.5 b) plus 0.75 (b - 1), so one sample's
    statistics used for another, or zero instead of replicate padding, cannot pass the gate."""
    x = synth.hash_unitvar(seed, (3 * N, C, D, H, W), stream=1)
    b = np.arange(3 * N, dtype=np.float32).reshape(-1, 1, 1, 1, 1)
    x = x * (np.float32(0.5) + np.float32(0.5) * b) + np.float32(0.75) * (b - np.float32(1.0))
    return np.ascontiguousarray(x.astype(np.float32).reshape(N, 3 * C * D, H, W))


def case_inputs(name):
    """(depth, state_dict, input [N, 3 C D, H, W] float32 numpy)."""
    N, D, H, W, alphas, seed_w, seed_x = CASES[name]
    return D, weights(seed_w, D, alphas), planes(seed_x, N, D, H, W)


def rel(a, b, scale=None):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() if scale is None else scale))


def hip_module(sd, D, dev):
    from real3dportrait_amd.plane2grid import Plane2GridModule
    m = Plane2GridModule(D, 3 * C)
    m.load_state_dict(sd, strict=True)
    return m.to(dev).eval()


class SameBlock3d(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.conv1 = nn.Conv3d(c, c, 3, padding=1, padding_mode="replicate")
        self.conv2 = nn.Conv3d(c, c, 3, padding=1, padding_mode="replicate")
        self.norm1, self.norm2 = nn.GroupNorm(GROUPS, c), nn.GroupNorm(GROUPS, c)
        self.alpha = nn.Parameter(torch.tensor([0.01]))

    def forward(self, x):
        return x + self.alpha * self.conv2(F.relu(self.norm2(self.conv1(F.relu(self.norm1(x))))))


class Plane2GridModule(nn.Module):
    """A plain-torch mock with the reference's class name, attributes (triplane_depth, in_out_dim, res_blocks_3d) and state_dict keys.
    A stand-in for the reference: the goldens come from the reference's own class (tests/golden/make_golden_plane2grid.py)."""

    def __init__(self, triplane_depth=3, in_out_dim=96):
        super().__init__()
        self.triplane_depth, self.in_out_dim = triplane_depth, in_out_dim
        self.num_layers_per_block = layers_for(triplane_depth)
        self.res_blocks_3d = nn.Sequential(*[SameBlock3d(in_out_dim // 3) for _ in range(self.num_layers_per_block)])

    def forward(self, x):
        N, _, H, W = x.shape
        D, c = self.triplane_depth, self.in_out_dim // 3
        return self.res_blocks_3d(x.reshape(N * 3, c, D, H, W)).reshape(N, 3 * c * D, H, W)


def mock_module(sd, D, in_out_dim=96):
    m = Plane2GridModule(D, in_out_dim)
    if sd is not None:
        m.load_state_dict(sd, strict=True)
    return m.eval()
