"""The two synthetic set-ups that scripts/ab_outputs.py and scripts/gpu_stamps.py share: the ray scene (two plane sets summed, the seed-7 decoder,
cameras 5.. of the 64-step sweep, hash noise, camera mode) and one SR block with its seeded weights and input.  Imports torch and the package:
for scripts that run on the GPU only."""
import functools

import numpy as np
import torch
from real3dportrait_amd import ImportanceRenderer, OSGDecoder, SynthesisBlock, synth

T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(None)
def _ray_scene():
    planes = T(synth.synth_planes(7, N=1) + synth.synth_planes(8, N=1, scale=0.1)); dn = synth.synth_decoder(7, sigma_bias=4.0)
    dec = OSGDecoder().cuda()
    with torch.no_grad():
        dec.net[0].weight.copy_(T(dn[0])); dec.net[0].bias.copy_(T(dn[1])); dec.net[2].weight.copy_(T(dn[2])); dec.net[2].bias.copy_(T(dn[3]))
    return planes, dec


def ray_case(R, Nc, Nf, N=1, **renderer):
    """call() -> the outputs of ImportanceRenderer.forward_camera for N cameras at R^2 rays, Nc + Nf samples; `renderer` sets attributes
    of the renderer (seed=77, need_depth=False)."""
    planes, dec = _ray_scene()
    cam = T(synth.camera_sweep(64, -0.4, 0.4)[5:5 + N])
    ren = ImportanceRenderer(hp={}); ren.noise_mode = "hash"
    for k, v in renderer.items(): setattr(ren, k, v)
    opts = {"ray_start": "auto", "ray_end": "auto", "box_warp": 1.0, "depth_resolution": Nc, "depth_resolution_importance": Nf,
            "disparity_space_sampling": False, "clamp_mode": "softplus", "white_back": False}
    nhwc = ren.prepare_planes(planes.expand(N, -1, -1, -1, -1).contiguous())
    return lambda: ren.forward_camera(nhwc, dec, cam[:, :16].view(-1, 4, 4), cam[:, 16:].view(-1, 3, 3), R, opts)


def sr_block(cin, cout, res, seed, prec):
    """call() -> one SynthesisBlock forward, cin -> cout channels, res^2 -> (2 res)^2, weights of synth_sr_block(7, .., seed), no noise."""
    blk = SynthesisBlock(cin, cout, w_dim=512, resolution=2 * res, img_channels=3, is_last=False, conv_clamp=None).cuda()
    blk.precision = prec
    p = synth.synth_sr_block(7, cin, cout, 512, seed)
    with torch.no_grad():
        for name in ("conv0", "conv1", "torgb"):
            l = getattr(blk, name); w, b, aw, ab = p[name]
            l.weight.copy_(T(w)); l.bias.copy_(T(b)); l.affine.weight.copy_(T(aw)); l.affine.bias.copy_(T(ab))
    x = T(synth.hash_unitvar(7, (1, cin, res, res), stream=1)); img = x[:, :3].contiguous(); ws = torch.ones(1, 3, 512, device="cuda")
    return lambda: blk(x, img, ws, noise_mode="none")
