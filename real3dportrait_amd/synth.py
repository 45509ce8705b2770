"""Deterministic synthetic inputs for tests and benchmarks (no checkpoints / datasets exist offline).

Everything is derived from a counter-based integer hash (splitmix64) evaluated in numpy, so the
same (seed, shape) gives bit-identical arrays in the build container, on the GPU box and on every
rank of a sharded run -- independent of torch / numpy RNG stream versions.

Shapes follow the reference: tri-planes [N,3,32,256,256] (modules/img2plane/img2plane_model.py:72-82),
decoder 32->64->33 (modules/eg3ds/models/triplane.py:166-176), SR parameter names of
SuperresolutionHybrid8XDC (modules/eg3ds/models/superresolution.py:331-346), camera = 16 c2w + 9
intrinsics floats (modules/eg3ds/camera_utils/pose_sampler.py:28-36; focal 4.2647, radius 2.7).
"""
import math

import numpy as np

_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def _splitmix64(x):
    x = (x + np.uint64(0x9E3779B97F4A7C15)) & _M64
    z = x
    z = ((z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)) & _M64
    z = ((z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)) & _M64
    return z ^ (z >> np.uint64(31))


def hash_uniform(seed, n, stream=0):
    """n float32 values in [0,1) with 24 random bits each."""
    with np.errstate(over="ignore"):
        base = _splitmix64(np.uint64(seed) * np.uint64(0x100000001B3) + np.uint64(stream))
        ctr = np.arange(n, dtype=np.uint64) + base
        bits = _splitmix64(ctr) >> np.uint64(40)
    return (bits.astype(np.float32) * np.float32(1.0 / (1 << 24))).astype(np.float32)


def hash_unitvar(seed, shape, stream=0):
    """Zero-mean unit-variance float32 array (Irwin-Hall sum of 4 uniforms; bounded, bell-shaped)."""
    n = int(np.prod(shape))
    u = hash_uniform(seed, 4 * n, stream).reshape(4, n)
    s = (u[0] + u[1]) + (u[2] + u[3])
    return ((s - np.float32(2.0)) * np.float32(math.sqrt(3.0))).astype(np.float32).reshape(shape)


def synth_noise(seed, shape, stream=7):
    return hash_uniform(seed, int(np.prod(shape)), stream).reshape(shape)


def synth_planes(seed, N=1, C=32, H=256, W=256, scale=1.0):
    return (hash_unitvar(seed, (N, 3, C, H, W), stream=1) * np.float32(scale)).astype(np.float32)


def synth_decoder(seed, C=32, HID=64, OUT=33, sigma_bias=0.0):
    """Raw OSGDecoder parameters (net.0.weight, net.0.bias, net.2.weight, net.2.bias).
    `sigma_bias` shifts the density pre-activation ("dense" variant of SURVEY 8d)."""
    w1 = hash_unitvar(seed, (HID, C), stream=11)
    b1 = hash_unitvar(seed, (HID,), stream=12) * np.float32(0.1)
    w2 = hash_unitvar(seed, (OUT, HID), stream=13)
    b2 = hash_unitvar(seed, (OUT,), stream=14) * np.float32(0.1)
    b2[0] += np.float32(sigma_bias)
    return w1, b1, w2, b2


def synth_sr_block(seed, cin, cout, w_dim=512, stream0=100):
    """conv0/conv1/torgb -> (weight, bias, affine.weight, affine.bias) like SynthesisBlock."""
    def layer(ci, co, k, s):
        return (hash_unitvar(seed, (co, ci, k, k), stream=s),
                hash_unitvar(seed, (co,), stream=s + 1) * np.float32(0.1),
                hash_unitvar(seed, (ci, w_dim), stream=s + 2),
                (np.ones((ci,), np.float32) + hash_unitvar(seed, (ci,), stream=s + 3) * np.float32(0.05)))
    return {"conv0": layer(cin, cout, 3, stream0),
            "conv1": layer(cout, cout, 3, stream0 + 10),
            "torgb": layer(cout, 3, 1, stream0 + 20)}


def synth_sr_params(seed, channels=32, mid=256, last=128, w_dim=512):
    """Parameters of SuperresolutionHybrid8XDC: block0 (channels->mid), block1 (mid->last)."""
    return [synth_sr_block(seed, channels, mid, w_dim, 100), synth_sr_block(seed, mid, last, w_dim, 200)]


# channel plans of the torso / background fusion stacks (modules/real3d/super_resolution/sr_with_ref.py:24-63):
# (in_channels, out_channels, kernel_size, leaky_relu_after)
FUSION_STACKS = {
    "torso_encoder": [(64, 256, 1, False)],
    "bg_encoder": [(3, 64, 3, True), (64, 256, 3, True), (256, 256, 3, False)],
    "fuse_head_torso_convs": [(512, 256, 3, True), (256, 256, 3, False)],
    "fuse_fg_bg_convs": [(512, 64, 1, True), (64, 256, 3, True), (256, 256, 3, False)],
}


# SegFormerSECC2PlaneBackbone.to_plane_cnn (modules/real3d/segformer.py:691-700); "up" = UpsamplingBilinear2d(2) before the conv
TO_PLANE_CNN = [(256, 256, 3, True), (256, 256, 3, True), (256, 256, 3, True), (256, 96, 3, False)]
TO_PLANE_CNN_UP_BEFORE = 3          # the x2 bilinear up-sampling sits in front of layer 3


def synth_conv_stack(seed, plan, stream0=300):
    """[(weight [co,ci,k,k], bias [co])] for a FUSION_STACKS plan; weights ~ N(0, 1/(ci k k)) so activations stay O(1)."""
    out = []
    for i, (ci, co, k, _) in enumerate(plan):
        w = hash_unitvar(seed, (co, ci, k, k), stream=stream0 + 2 * i) * np.float32(1.0 / math.sqrt(ci * k * k))
        b = hash_unitvar(seed, (co,), stream=stream0 + 2 * i + 1) * np.float32(0.1)
        out.append((w.astype(np.float32), b.astype(np.float32)))
    return out


def look_at_camera(yaw=0.0, pitch=0.0, radius=2.7, lookat=(0.0, 0.0, 0.2), focal=4.2647):
    """camera[25] = flattened OpenCV-convention cam2world (4x4) + normalised intrinsics (3x3)."""
    la = np.asarray(lookat, np.float64)
    origin = la + radius * np.array([math.sin(yaw) * math.cos(pitch), math.sin(pitch),
                                     math.cos(yaw) * math.cos(pitch)])
    fwd = la - origin
    fwd /= np.linalg.norm(fwd)
    up = np.array([0.0, 1.0, 0.0])
    right = -np.cross(up, fwd)
    right /= np.linalg.norm(right)
    up2 = np.cross(fwd, right)
    up2 /= np.linalg.norm(up2)
    c2w = np.eye(4)
    c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = right, up2, fwd, origin
    K = np.array([[focal, 0, 0.5], [0, focal, 0.5], [0, 0, 1.0]])
    return np.concatenate([c2w.reshape(-1), K.reshape(-1)]).astype(np.float32)


def camera_sweep(n, yaw_lo=-0.4, yaw_hi=0.4, pitch=0.0):
    yaws = np.linspace(yaw_lo, yaw_hi, n) if n > 1 else np.array([0.0])
    return np.stack([look_at_camera(float(y), pitch) for y in yaws]).astype(np.float32)


# ---- host mirror of the device's counter-based sampling noise (csrc/r3d_common.h: mix32 / hash_uniform) ---------------------------
# noise_mode='hash' of ImportanceRenderer replaces the two RNG draws of the reference (torch.rand_like at
# modules/eg3ds/volumetric_rendering/renderer.py:226, torch.rand at :281) by a function of (seed, stream, index): stream 0 = the coarse
# jitter, index = ray * Nc + k; stream 1 = the importance u, index = ray * Nf + j; ray = n * M + m.  tests/test_gpu_pinned_config.py
# holds this mirror bit-identical to the kernel (hash mode == the same arrays injected) and feeds them to the oracle.
def _mix32(x):
    x = x.astype(np.uint32)
    x ^= x >> np.uint32(16)
    x = (x * np.uint32(0x7FEB352D)).astype(np.uint32)
    x ^= x >> np.uint32(15)
    x = (x * np.uint32(0x846CA68B)).astype(np.uint32)
    x ^= x >> np.uint32(16)
    return x


def device_hash_uniform(seed, stream, idx):
    """float32 [0,1) values of r3d::hash_uniform(seed, stream, idx) for an array of 64-bit indices."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    idx = np.asarray(idx, dtype=np.uint64)
    with np.errstate(over="ignore"):
        h0 = np.uint32((seed & 0xFFFFFFFF) ^ ((0x9E3779B9 * (int(stream) + 1)) & 0xFFFFFFFF))
        h = _mix32(np.full(1, h0, np.uint32))
        h = _mix32(h ^ np.uint32(seed >> 32))
        h = _mix32(h ^ (idx & np.uint64(0xFFFFFFFF)).astype(np.uint32))
        h = _mix32(h ^ (idx >> np.uint64(32)).astype(np.uint32) ^ np.uint32(0x85EBCA6B))
    return ((h >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)).astype(np.float32)


def render_hash_noise(seed, rays, Nc, Nf):
    """(noise_coarse [len(rays), Nc], u_fine [len(rays), Nf]) the ray kernel derives for the global ray indices `rays` (n * M + m)."""
    rays = np.asarray(rays, dtype=np.uint64).reshape(-1, 1)
    nc = device_hash_uniform(seed, 0, rays * np.uint64(Nc) + np.arange(Nc, dtype=np.uint64)[None, :])
    uf = device_hash_uniform(seed, 1, rays * np.uint64(max(Nf, 1)) + np.arange(max(Nf, 1), dtype=np.uint64)[None, :])[:, :Nf]
    return nc, uf


# ---- surface-like scenes for the ray kernel (what a trained checkpoint looks like to the renderer) --------------------------------
def surface_scene(seed, N=1, H=64, W=64, centre=(0.15, 0.1, 0.05), radius=0.3, a=100.0, c=None, bg_bias=-5.0, box_warp=1.0,
                  triplane_depth=1, dense=False, texture=0.3):
    """(planes [N,3,32*D,H,W], (w1, b1, w2, b2)) of an opaque textured sphere in near-empty space.

    The random planes of synth_planes give every ray a weight sum of 0.3-1 spread along its whole length.  A trained model
    packs density onto a surface instead: transmittance falls to ~0 at the hit, the space around it is near-empty, and the
    importance samples crowd into one or two coarse bins.  This scene has that shape with a closed-form surface:

    * Feature channel 0 is a quadratic sampled at the texel centres (grid_sample, align_corners=False: texel i of n sits at
      (2i+1)/n - 1).  With the plane axes of renderer.py:37-63 (plane 0 reads (x, y), plane 1 (x, z), plane 2 (z, x), in
      coordinates scaled by 2/box_warp, renderer.py:71), plane 0 holds (u-qx)^2 + (v-qy)^2, plane 1 holds (v-qz)^2 and
      plane 2 holds 0, so the decoder's plane mean (triplane.py:179) is s = |q - qc|^2 / 3 for q = 2p/box_warp.  Tri-grids
      (triplane_depth D > 1) hold the same value at every depth slice.
    * The other 31 channels are `texture` * hash_unitvar noise (the colour texture).
    * Hidden unit 0 of the decoder is softplus(a (s0 - s)) with s0 = (2 radius / box_warp)^2 / 3: w1[0] = e0 * (-a sqrt(C))
      and b1[0] = a s0 undo FullyConnectedLayer's weight gain 1/sqrt(C) (networks_stylegan2.py:99-131).  No other hidden
      unit reads channel 0.  The surface is a steep softplus, not a large bias cancelled in layer 2 (that would measure
      fp32 rounding of the bias, not the renderer).
    * The density row reads only that unit: w2[0] = e0 * c sqrt(HID) (gain 1/sqrt(HID)), b2[0] = bg_bias; so sigma =
      c softplus(a (s0 - s)) + bg_bias, and MipRayMarcher2's softplus(sigma - 1) (ray_marcher.py:25-57) gives ~e^(bg_bias-1)
      outside the sphere and ~c a (s0 - s) inside.  The rgb rows are synth_decoder's.
    * dense=True raises c from 30 to 600: sigma * delta > 20 inside at 48 coarse samples, so 1 - exp(-sigma delta) rounds
      to 1 in fp32 and the transmittance products underflow.

    `centre` (world units) is off the box centre so that the silhouette crosses the image of look_at_camera.  Everything is
    computed in float64 numpy from the parameters and rounded once to float32: bit-reproducible on every machine."""
    C, HID, OUT = 32, 64, 33
    D = int(triplane_depth)
    if c is None:
        c = 600.0 if dense else 30.0
    qc = [2.0 * float(x) / float(box_warp) for x in centre]
    s0 = (2.0 * float(radius) / float(box_warp)) ** 2 / 3.0
    planes = hash_unitvar(seed, (N, 3, C * D, H, W), stream=41) * np.float32(texture)
    u = (2.0 * np.arange(W, dtype=np.float64) + 1.0) / W - 1.0        # texel centres along the width axis (first coordinate)
    v = (2.0 * np.arange(H, dtype=np.float64) + 1.0) / H - 1.0        # ... along the height axis (second coordinate)
    ch0 = np.zeros((3, H, W), np.float64)
    ch0[0] = (u[None, :] - qc[0]) ** 2 + (v[:, None] - qc[1]) ** 2   # plane 0: (x, y)
    ch0[1] = np.broadcast_to((v[:, None] - qc[2]) ** 2, (H, W))       # plane 1: (x, z) -> z is the second coordinate
    planes[:, :, 0:D] = ch0.astype(np.float32)[None, :, None]         # channel 0 = channels 0..D-1 of the [C*D] layout
    w1, b1, w2, b2 = synth_decoder(seed, C, HID, OUT)
    w1[:, 0] = 0.0
    w1[0, :] = 0.0
    w1[0, 0] = np.float32(-float(a) * math.sqrt(C))
    b1[0] = np.float32(float(a) * s0)
    w2[0, :] = 0.0
    w2[0, 0] = np.float32(float(c) * math.sqrt(HID))
    b2[0] = np.float32(bg_bias)
    return planes.astype(np.float32), (w1, b1, w2, b2)


SECC_DIMS, SECC_HEADS, SECC_SR = (32, 64, 160, 256), (1, 2, 5, 8), (8, 4, 2, 1)     # mit_b0 (modules/real3d/segformer.py:407-413)


def secc_backbone_shapes(pncc_cond_mode="cano_src_tgt", out_channels=96):
    """[(state_dict key, shape)] of SegFormerSECC2PlaneBackbone('b0', out_channels, pncc_cond_mode) (modules/real3d/segformer.py:672-700)."""
    in_dim = 9 if pncc_cond_mode == "cano_src_tgt" else 6
    out = [("prenet.weight", (3, in_dim, 1, 1)), ("prenet.bias", (3,)), ("prenet.resample_filter", (4, 4))]
    cin = 3
    for s, (C, sr) in enumerate(zip(SECC_DIMS, SECC_SR), 1):
        k = 7 if s == 1 else 3
        p = "mix_vit.patch_embed%d." % s
        out += [(p + "proj.weight", (C, cin, k, k)), (p + "proj.bias", (C,)), (p + "norm.weight", (C,)), (p + "norm.bias", (C,))]
        for j in range(2):
            p = "mix_vit.block%d.%d." % (s, j)
            out += [(p + "norm1.weight", (C,)), (p + "norm1.bias", (C,)), (p + "attn.q.weight", (C, C)), (p + "attn.q.bias", (C,)),
                    (p + "attn.kv.weight", (2 * C, C)), (p + "attn.kv.bias", (2 * C,)), (p + "attn.proj.weight", (C, C)),
                    (p + "attn.proj.bias", (C,))]
            if sr > 1:
                out += [(p + "attn.sr.weight", (C, C, sr, sr)), (p + "attn.sr.bias", (C,)), (p + "attn.norm.weight", (C,)),
                        (p + "attn.norm.bias", (C,))]
            out += [(p + "norm2.weight", (C,)), (p + "norm2.bias", (C,)), (p + "mlp.fc1.weight", (4 * C, C)), (p + "mlp.fc1.bias", (4 * C,)),
                    (p + "mlp.dwconv.dwconv.weight", (4 * C, 1, 3, 3)), (p + "mlp.dwconv.dwconv.bias", (4 * C,)),
                    (p + "mlp.fc2.weight", (C, 4 * C)), (p + "mlp.fc2.bias", (C,))]
        out += [("mix_vit.norm%d.weight" % s, (C,)), ("mix_vit.norm%d.bias" % s, (C,))]
        cin = C
    for s, C in enumerate(SECC_DIMS, 1):
        out += [("fuse_head.linear_c%d.proj.weight" % s, (256, C)), ("fuse_head.linear_c%d.proj.bias" % s, (256,))]
    out += [("fuse_head.linear_fuse.conv.weight", (256, 1024, 1, 1))]
    out += [("fuse_head.linear_fuse.bn." + n, (256,)) for n in ("weight", "bias", "running_mean", "running_var")]
    out += [("fuse_head.linear_fuse.bn.num_batches_tracked", ())]
    for i, co in ((0, 256), (2, 256), (4, 256), (7, out_channels)):
        out += [("to_plane_cnn.%d.weight" % i, (co, 256, 3, 3)), ("to_plane_cnn.%d.bias" % i, (co,))]
    return out


def synth_secc_backbone(seed, pncc_cond_mode="cano_src_tgt", out_channels=96, qk_gain=2.5):
    """A full state_dict (numpy) of SegFormerSECC2PlaneBackbone('b0') from hash_unitvar streams, scaled so that activations stay O(1)
    through every stage: weights ~ N(0, 1/fan_in) (the prenet's raw weight unit variance: Conv2dLayer applies 1/sqrt(fan_in) itself),
    biases 0.1 n, LayerNorm / BatchNorm weights 1 + 0.1 n, BN running_var in [0.5, 2].  The q weights and the key half of the kv weights
    carry `qk_gain`, so that the attention logits reach about +-20 (a peaked softmax, not a uniform one)."""
    sd = {}
    for i, (key, shape) in enumerate(secc_backbone_shapes(pncc_cond_mode, out_channels)):
        st = 1000 + i
        last = key.rsplit(".", 1)[-1]
        if key == "prenet.resample_filter":
            f = np.array([1.0, 3.0, 3.0, 1.0], np.float32)
            v = np.outer(f, f) / np.float32(64.0)                  # upfirdn2d.setup_filter([1, 3, 3, 1])
        elif last == "num_batches_tracked":
            v = np.array(0, dtype=np.int64)
        elif last == "running_var":
            v = np.float32(0.5) + np.float32(1.5) * hash_uniform(seed, shape[0], st)
        elif last in ("bias", "running_mean"):
            v = hash_unitvar(seed, shape, st) * np.float32(0.1)
        elif len(shape) == 1:                                        # LayerNorm / BatchNorm weight
            v = np.float32(1.0) + hash_unitvar(seed, shape, st) * np.float32(0.1)
        else:
            fan_in = int(np.prod(shape[1:]))
            v = hash_unitvar(seed, shape, st) * np.float32(1.0 if key == "prenet.weight" else 1.0 / math.sqrt(fan_in))
            if key.endswith("attn.q.weight"):
                v = v * np.float32(qk_gain)
            elif key.endswith("attn.kv.weight"):
                v[: shape[0] // 2] *= np.float32(qk_gain)
        sd[key] = np.asarray(v, dtype=np.int64 if last == "num_batches_tracked" else np.float32)
    return sd


IMG2PLANE_BLOCKS = {"small": (2, 1), "standard": (5, 1), "large": (10, 3)}      # (LowResolutionViT, TriplanePredictorViT) blocks, segformer/models.py


def img2plane_shapes(scale="standard", in_channels=5, out_channels=96):
    """[(state_dict key, shape)] of Img2PlaneModel (modules/img2plane/img2plane_model.py:12-35) without low_reso_encoder.*: in_channels is
    what the two encoders read, the mode's channels + 2 (rgb 5, rgb_alpha 6, rgb_camera 8, rgb_alpha_camera 9); 8 and 9 carry
    camera_to_channel."""
    out = [("camera_to_channel.weight", (3, 25)), ("camera_to_channel.bias", (3,))] if in_channels in (8, 9) else []
    conv = lambda p, co, ci, k: [(p + ".weight", (co, ci, k, k)), (p + ".bias", (co,))]
    lin = lambda p, co, ci: [(p + ".weight", (co, ci)), (p + ".bias", (co,))]
    norm = lambda p: [(p + ".weight", (1024,)), (p + ".bias", (1024,))]

    def block(p, sr):
        b = norm(p + "norm1") + lin(p + "attn.q", 1024, 1024) + lin(p + "attn.kv", 2048, 1024) + lin(p + "attn.proj", 1024, 1024)
        if sr > 1:
            b += conv(p + "attn.sr", 1024, 1024, sr) + norm(p + "attn.norm")
        return (b + norm(p + "norm2") + lin(p + "mlp.fc1", 2048, 1024) + [(p + "mlp.dwconv.dwconv.weight", (2048, 1, 3, 3)), (p + "mlp.dwconv.dwconv.bias", (2048,))]
                + lin(p + "mlp.fc2", 1024, 2048))

    n_low, n_pred = IMG2PLANE_BLOCKS[scale]
    p = "high_reso_encoder."
    out += conv(p + "first", 64, in_channels, 7) + conv(p + "conv_layers.0", 96, 64, 3)
    for i in (2, 4, 6):
        out += conv(p + "conv_layers.%d" % i, 96, 96, 3)
    out += conv(p + "final", 96, 96, 3)
    p = "low_reso_vit."
    out += conv(p + "patch_embed.proj", 1024, 256, 3) + norm(p + "patch_embed.norm")
    for i in range(1, n_low + 1):
        out += block(p + "block%d." % i, 1)
    out += conv(p + "conv_after_upsample1", 128, 256, 3) + conv(p + "conv_after_upsample2", 128, 128, 3) + conv(p + "final_conv", 96, 128, 3)
    p = "triplane_predictor_vit."
    out += conv(p + "first_conv", 256, 192, 3) + conv(p + "second_conv", 128, 256, 3)
    out += conv(p + "patch_embed.proj", 1024, 128, 3) + norm(p + "patch_embed.norm")
    for i in range(1, n_pred + 1):
        out += block(p + "block%d." % i, 2)
    out += conv(p + "first_conv_after_cat", 256, 352, 3) + conv(p + "second_conv_after_cat", 128, 256, 3)
    out += conv(p + "third_conv_after_cat", 128, 128, 3) + conv(p + "final_conv", out_channels, 128, 3)
    return out


def synth_img2plane(seed, scale="standard", in_channels=5, qk_gain=1.5, out_channels=96):
    """A state_dict (numpy) of Img2PlaneModel without low_reso_encoder.*, from hash_unitvar streams as synth_secc_backbone makes its own:
    weights ~ N(0, gain / fan_in) with gain 2 in front of a ReLU / LeakyReLU / GELU and 1 elsewhere, biases 0.1 n, LayerNorm weights
    1 + 0.1 n.  The q weights and the key half of the kv weights carry `qk_gain`: with LayerNorm-ed inputs the logits' spread is about
    qk_gain^2, a softmax that is neither uniform nor one-hot at 16 .. 4096 keys."""
    relu_fed = ("conv_layers", "conv_after_upsample", "first_conv", "second_conv", "third_conv", "mlp.fc1", "mlp.dwconv")
    sd = {}
    for i, (key, shape) in enumerate(img2plane_shapes(scale, in_channels, out_channels)):
        st = 5000 + i
        last = key.rsplit(".", 1)[-1]
        if last == "bias":
            v = hash_unitvar(seed, shape, st) * np.float32(0.1)
        elif len(shape) == 1:
            v = np.float32(1.0) + hash_unitvar(seed, shape, st) * np.float32(0.1)
        else:
            fan_in = int(np.prod(shape[1:]))
            gain = 2.0 if any(n in key for n in relu_fed) else 1.0
            v = hash_unitvar(seed, shape, st) * np.float32(math.sqrt(gain / fan_in))
            if key.endswith("attn.q.weight"):
                v = v * np.float32(qk_gain)
            elif key.endswith("attn.kv.weight"):
                v[: shape[0] // 2] *= np.float32(qk_gain)
        sd[key] = np.asarray(v, dtype=np.float32)
    return sd


DEEPLAB_LAYERS = {"resnet18": (2, 2, 2, 2), "resnet34": (3, 4, 6, 3)}


def deeplabv3_shapes(in_channels=5, encoder_name="resnet34", decoder_channels=256):
    """[(state_dict key, shape)] of DeepLabV3 (modules/img2plane/deeplabv3/decoders/my_model.py) over a BasicBlock ResNet, in the order
    of its state_dict; BatchNorm's num_batches_tracked (shape ()) included."""
    conv = lambda p, co, ci, k: [(p + ".weight", (co, ci, k, k))]
    bn = lambda p, c: [(p + ".weight", (c,)), (p + ".bias", (c,)), (p + ".running_mean", (c,)), (p + ".running_var", (c,)),
                       (p + ".num_batches_tracked", ())]
    out = conv("encoder.conv1", 64, in_channels, 7) + bn("encoder.bn1", 64)
    inplanes = 64
    for i, (planes, n) in enumerate(zip((64, 128, 256, 512), DEEPLAB_LAYERS[encoder_name])):
        for j in range(n):
            p = "encoder.layer%d.%d." % (i + 1, j)
            cin = inplanes if j == 0 else planes
            out += conv(p + "conv1", planes, cin, 3) + bn(p + "bn1", planes) + conv(p + "conv2", planes, planes, 3) + bn(p + "bn2", planes)
            if j == 0 and i > 0:
                out += conv(p + "downsample.0", planes, cin, 1) + bn(p + "downsample.1", planes)
        inplanes = planes
    C = decoder_channels
    out += conv("decoder.0.convs.0.0", C, 512, 1)
    for i in (1, 2, 3):
        out += conv("decoder.0.convs.%d.0" % i, C, 512, 3)
    out += conv("decoder.0.convs.4.1", C, 512, 1) + conv("decoder.0.project.0", C, 5 * C, 1) + conv("decoder.1", C, C, 3)
    return out


def synth_deeplabv3(seed, in_channels=5, encoder_name="resnet34"):
    """A state_dict (numpy) of DeepLabV3 from hash streams, as the other synth_* functions make theirs: conv weights ~ N(0, gain / fan_in)
    with gain 2 (He) and 0.5 on each block's second conv, on the downsample convs and on the last conv; BatchNorm weight 1 + 0.1 n, bias
    and running mean 0.1 n, running variance 1 .. 1.2, num_batches_tracked 0.  With these every ReLU of the network passes a middling
    share of its elements and no stage's magnitude runs away (the golden maker asserts both)."""
    sd = {}
    for i, (key, shape) in enumerate(deeplabv3_shapes(in_channels, encoder_name)):
        st = 5600 + i
        last = key.rsplit(".", 1)[-1]
        if last == "num_batches_tracked":
            v = np.zeros((), np.int64)
        elif last == "running_var":
            v = np.float32(1.0) + hash_uniform(seed, int(np.prod(shape)), st).reshape(shape) * np.float32(0.2)
        elif last in ("bias", "running_mean"):
            v = hash_unitvar(seed, shape, st) * np.float32(0.1)
        elif len(shape) == 1:
            v = np.float32(1.0) + hash_unitvar(seed, shape, st) * np.float32(0.1)
        else:
            small = ".conv2." in key or "downsample" in key or key.startswith("decoder.1.")
            v = hash_unitvar(seed, shape, st) * np.float32(math.sqrt((0.5 if small else 2.0) / int(np.prod(shape[1:]))))
        sd[key] = np.asarray(v, dtype=np.int64 if last == "num_batches_tracked" else np.float32)
    return sd


TORSO_C, TORSO_D = 32, 16          # the appearance volume [N, 32, 16, H, W] (facev2v_warp/network2.py:248-256)


def torso_generator_shapes():
    """[(state_dict key, shape)] of Generator() at standard / small scale (modules/real3d/facev2v_warp/network2.py:248-280): 139 entries."""
    sn = lambda p, co, ci, k: [(p + "bias", (co,)), (p + "weight_orig", (co, ci, k, k)), (p + "weight_u", (co,)), (p + "weight_v", (ci * k * k,))]
    bn = lambda p, c: [(p + n, (c,)) for n in ("weight", "bias", "running_mean", "running_var")] + [(p + "num_batches_tracked", ())]
    out = sn("in_conv.layers.0.", 256, TORSO_C * TORSO_D, 3) + bn("in_conv.layers.1.", 256)
    out += [("mid_conv.weight", (256, 256, 1, 1)), ("mid_conv.bias", (256,))]
    for i in range(6):
        for j in range(2):
            p = "res.%d.layers.%d.layers." % (i, j)
            out += bn(p + "0.", 256) + sn(p + "2.", 256, 256, 3)
    for i, (ci, co) in enumerate(((256, 128), (128, 64))):
        p = "up.%d.layers.1.layers." % i
        out += sn(p + "0.", co, ci, 3) + bn(p + "1.", co)
    return out + [("out_conv.weight", (3, 64, 7, 7)), ("out_conv.bias", (3,))]


def torso_predictor_shapes():
    """occlusion_2_predictor (facev2v_warp/model2.py:212-219)."""
    out = []
    for i, (ci, co) in zip((0, 2, 4), ((65, 32), (32, 32), (32, 1))):
        out += [("%d.weight" % i, (co, ci, 3, 3)), ("%d.bias" % i, (co,))]
    return out


def synth_torso_generator(seed):
    """A full state_dict (numpy) of the torso Generator.  Conv weights ~ N(0, gain^2 / fan_in); a spectral-normed conv's gain alternates
    between 0.5 and 2 from layer to layer, so that sigma is far from 1 everywhere (the effective weight, weight_orig / sigma, does not
    depend on it).  weight_u / weight_v come from one power iteration on weight_orig started at a hash vector, then perturbed by 10 %:
    random u, v would make sigma tiny and the activations astronomically large.  BatchNorm: weight 1.5 (1 + 0.1 n) (it makes up for the
    1 / sigma and the ReLU in front of each conv), bias and running_mean 0.3 n, running_var in [0.5, 2]."""
    sd = {}
    shapes = torso_generator_shapes()
    n_sn = 0
    for i, (key, shape) in enumerate(shapes):
        st = 3000 + i
        last = key.rsplit(".", 1)[-1]
        if last in ("weight_u", "weight_v"):
            continue                                                 # with their weight_orig
        if last == "num_batches_tracked":
            v = np.array(0, dtype=np.int64)
        elif last == "running_var":
            v = np.float32(0.5) + np.float32(1.5) * hash_uniform(seed, shape[0], st)
        elif last == "running_mean" or (last == "bias" and len(shape) == 1 and (key[:-4] + "running_mean") in dict(shapes)):
            v = hash_unitvar(seed, shape, st) * np.float32(0.3)
        elif last == "bias":
            v = hash_unitvar(seed, shape, st) * np.float32(0.1)
        elif len(shape) == 1:                                        # BatchNorm weight
            v = np.float32(1.5) * (np.float32(1.0) + hash_unitvar(seed, shape, st) * np.float32(0.1))
        else:
            fan_in = int(np.prod(shape[1:]))
            v = hash_unitvar(seed, shape, st) * np.float32(1.0 / math.sqrt(fan_in))
            if last == "weight_orig":
                v = v * np.float32(2.0 if n_sn % 2 else 0.5)
                n_sn += 1
                wm = v.reshape(shape[0], -1).astype(np.float64)
                unit = lambda a: a / np.linalg.norm(a)
                v0 = unit(hash_unitvar(seed, (wm.shape[1],), st + 500).astype(np.float64))
                u = unit(wm @ v0)
                vv = unit(wm.T @ u)
                u = unit(u + 0.1 * hash_unitvar(seed, u.shape, st + 1000) / math.sqrt(u.size))
                vv = unit(vv + 0.1 * hash_unitvar(seed, vv.shape, st + 1500) / math.sqrt(vv.size))
                sd[key[:-4] + "u"], sd[key[:-4] + "v"] = u.astype(np.float32), vv.astype(np.float32)
        sd[key] = np.asarray(v, dtype=np.int64 if last == "num_batches_tracked" else np.float32)
    return {k: sd[k] for k, _ in shapes}


def synth_torso_predictor(seed):
    """occlusion_2_predictor's state_dict: weights ~ N(0, 2 / fan_in) (the first conv's, which reads a non-negative hid at rms of 6 or so,
    N(0, 0.05 / fan_in)), biases 0.1 n: the output logits stay O(1), a sigmoid that is neither saturated nor flat."""
    sd = {}
    for i, (key, shape) in enumerate(torso_predictor_shapes()):
        if len(shape) == 1:
            sd[key] = hash_unitvar(seed, shape, 3400 + i) * np.float32(0.1)
        else:
            sd[key] = hash_unitvar(seed, shape, 3400 + i) * np.float32(math.sqrt((0.05 if i == 0 else 2.0) / int(np.prod(shape[1:]))))
    return sd


def synth_torso_inputs(seed, N=1, H=64, W=64, noise=0.15):
    """Inputs of WarpBasedTorsoModelMediaPipe.infer_forward_stage2 and of the forward tail after it (facev2v_warp/model2.py:260-263):
    torso_appearance_feats [N, 32, 16, H, W] (unit variance), deformation [N, 16, H, W, 3] = the identity grid of align_corners=True + a
    smooth field of amplitude 0.1 + `noise` x N(0, 1), with a few rows forced to exactly -1, exactly 1 and exactly the identity (on source
    nodes), occlusion [N, 1, H, W] and the low-resolution occlusion_2 [N, 1, H, W] in [0, 1].  Every sample differs."""
    D = TORSO_D
    fs = hash_unitvar(seed, (N, TORSO_C, D, H, W), stream=11)
    lin = lambda n: (np.linspace(-1.0, 1.0, n) if n > 1 else np.zeros(1)).astype(np.float32)
    ident = np.stack(np.broadcast_arrays(lin(W)[None, None, :], lin(H)[None, :, None], lin(D)[:, None, None]), axis=-1).astype(np.float32)
    zz, yy, xx = np.meshgrid(lin(D), lin(H), lin(W), indexing="ij")
    grid = np.empty((N, D, H, W, 3), np.float32)
    for n in range(N):
        smooth = np.stack([np.sin(2.0 * yy + 3.0 * zz + n), np.cos(2.5 * xx - zz + 2 * n), np.sin(1.5 * xx + 2.0 * yy - n)], axis=-1)
        grid[n] = ident + np.float32(0.1) * smooth.astype(np.float32) + np.float32(noise) * hash_unitvar(seed, (D, H, W, 3), stream=12 + 10 * n)
    grid[:, 0, 0, :, :] = ident[0, 0]                  # exactly on source nodes
    grid[:, -1, -1, :, :] = ident[-1, -1]
    grid[:, D // 2, H // 2, : W // 2, :] = -1.0
    grid[:, D // 2, H // 2, W // 2:, :] = 1.0
    occ = hash_uniform(seed, N * H * W, stream=13).reshape(N, 1, H, W)
    occ2 = hash_uniform(seed, N * H * W, stream=14).reshape(N, 1, H, W)
    return {"torso_appearance_feats": fs, "deformation": grid, "occlusion": occ, "occlusion_2": occ2}


MOTION_D, MOTION_HW = 16, 64       # the estimator's fixed feature grid (facev2v_warp/network2.py:162-173, 220-222)


def torso_motion_shapes(K=4, input_channels=34):
    """[(state_dict key, shape)] of MotionFieldEstimator('standard', input_channels, K) (modules/real3d/facev2v_warp/network2.py:174-202):
    129 entries."""
    bn = lambda p, c: [(p + n, (c,)) for n in ("weight", "bias", "running_mean", "running_var")] + [(p + "num_batches_tracked", ())]
    conv = lambda p, co, ci, *k: [(p + "weight", (co, ci) + k), (p + "bias", (co,))]
    down, up = [5 * (K + 1), 64, 128, 256, 512, 1024], [1024, 512, 256, 128, 64, 32]
    out = conv("compress.", 4, input_channels, 1, 1, 1)
    for i in range(5):
        out += conv("down.%d.layers.0.layers.0." % i, down[i + 1], down[i], 3, 3, 3) + bn("down.%d.layers.0.layers.1." % i, down[i + 1])
    for i in range(5):
        out += conv("up.%d.layers.1.layers.0." % i, up[i + 1], up[i], 3, 3, 3) + bn("up.%d.layers.1.layers.1." % i, up[i + 1])
    out += conv("tgt_head_encoder.0.layers.0.", 32, 4, 7, 7) + bn("tgt_head_encoder.0.layers.1.", 32)
    for i in range(1, 4):
        for j in range(2):
            p = "tgt_head_encoder.%d.layers.%d.layers." % (i, j)
            out += bn(p + "0.", 32) + conv(p + "2.", 32, 32, 3, 3)
    out += conv("tgt_head_fuser.", 32, 32 + down[0] + 32, 7, 7, 7) + conv("mask_conv.", K + 1, 32, 7, 7, 7)
    return out + conv("occlusion_conv.", 1, 32 * MOTION_D, 7, 7) + conv("occlusion_conv2.", 1, 32 * MOTION_D, 7, 7)


# weight gains of synth_torso_motion (x 1 / sqrt(fan_in)), chosen so that on synth_torso_motion_inputs every activation stays O(1), the three
# channel groups of the fuser's input all matter, the mask's softmax is decided in places and open in others and the occlusions are neither
# saturated nor flat (tests/golden/make_golden_torso_motion.py asserts all of it on the reference's output)
MOTION_GAINS = {"compress": 1.0, "down": 2.0, "up": 1.6, "tgt_head_encoder.0": 2.0, "tgt_head_encoder": 1.0, "tgt_head_fuser": 1.0,
                "mask_conv": 4.0, "occlusion_conv": 0.8, "occlusion_conv2": 0.8}


def synth_torso_motion(seed, K=4, input_channels=34):
    """A full state_dict (numpy) of the motion-field estimator.  Conv weights ~ N(0, gain^2 / fan_in) with MOTION_GAINS by module, biases
    0.1 n (0.3 n in front of a BatchNorm); BatchNorm: weight 1 + 0.1 n, bias
    and running_mean 0.3 n, running_var in [0.5, 2]."""
    sd = {}
    shapes = torso_motion_shapes(K, input_channels)
    names = dict(shapes)
    for i, (key, shape) in enumerate(shapes):
        st = 4000 + i
        last = key.rsplit(".", 1)[-1]
        if last == "num_batches_tracked":
            v = np.array(0, dtype=np.int64)
        elif last == "running_var":
            v = np.float32(0.5) + np.float32(1.5) * hash_uniform(seed, shape[0], st)
        elif last == "running_mean":
            v = hash_unitvar(seed, shape, st) * np.float32(0.3)
        elif len(shape) == 1 and (key[:-len(last)] + "running_mean") in names:           # BatchNorm weight / bias
            v = hash_unitvar(seed, shape, st) * np.float32(0.3) if last == "bias" else np.float32(1.0) + hash_unitvar(seed, shape, st) * np.float32(0.1)
        elif last == "bias":
            front = key[:-6].rsplit(".", 1)[0] + ".1.running_mean" in names              # a "CNA" conv: its bias meets the BatchNorm's mean
            v = hash_unitvar(seed, shape, st) * np.float32(0.3 if front else 0.1)
        else:
            gain = next(g for p, g in MOTION_GAINS.items() if key.startswith(p))
            v = hash_unitvar(seed, shape, st) * np.float32(gain / math.sqrt(int(np.prod(shape[1:]))))
            if key == "mask_conv.weight":          # no response to a channel's mean: otherwise one component's logit leads everywhere
                v = v - v.mean(axis=(2, 3, 4), keepdims=True)
        sd[key] = np.asarray(v, dtype=np.int64 if last == "num_batches_tracked" else np.float32)
    return sd


def _rotation(yaw, pitch, roll):
    cy, sy, cp, sp, cr, sr = math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch), math.cos(roll), math.sin(roll)
    ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    rz = np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1]])
    return (rz @ ry @ rx).astype(np.float32)


def synth_torso_motion_inputs(seed, N=1, K=4, rotate=False):
    """Inputs of MotionFieldEstimator.forward as WarpBasedTorsoModelMediaPipe.forward passes them (facev2v_warp/model2.py:236-250):
    fs [N, 34, 16, 64, 64] (unit variance), kp_s / kp_d [N, K, 3] inside the volume (|kp_s| <= 0.55, kp_d = kp_s + an offset of 0.1 .. 0.3
    per axis with alternating signs, so that a good part of every sparse motion leaves the volume on one side or the other), Rs / Rd [N, 3, 3]
    (the identity as in the product, or with rotate two different rotations of up to 0.35 rad per axis), tgt_head_img [N, 3, 256, 256] in
    [-1, 1] (a smooth pattern + noise) and tgt_head_weights [N, 1, 256, 256] in [0, 1].  Every sample differs."""
    D, S = MOTION_D, MOTION_HW
    fs = hash_unitvar(seed, (N, 34, D, S, S), stream=21)
    kp_s = (hash_uniform(seed, N * K * 3, stream=22).reshape(N, K, 3) * np.float32(1.1) - np.float32(0.55)).astype(np.float32)
    u = hash_uniform(seed, N * K * 3, stream=23).reshape(N, K, 3)
    n_, k_, a_ = np.meshgrid(np.arange(N), np.arange(K), np.arange(3), indexing="ij")
    sign = np.where((n_ + k_ + a_) % 2 == 0, 1.0, -1.0)                # both signs on every axis
    kp_d = (kp_s + sign * (0.1 + 0.2 * u)).astype(np.float32)
    Rs = np.tile(np.eye(3, dtype=np.float32), (N, 1, 1))
    Rd = Rs.copy()
    if rotate:
        a = hash_uniform(seed, N * 6, stream=25).reshape(N, 6) * 0.7 - 0.35
        for n in range(N):
            Rs[n], Rd[n] = _rotation(*a[n, :3]), _rotation(*a[n, 3:])
    lin = np.linspace(-1.0, 1.0, 256, dtype=np.float32)
    yy, xx = np.meshgrid(lin, lin, indexing="ij")
    img = np.empty((N, 3, 256, 256), np.float32)
    wts = np.empty((N, 1, 256, 256), np.float32)
    for n in range(N):
        for c in range(3):
            img[n, c] = 0.6 * np.sin(3.0 * xx * (c + 1) + 2.0 * yy + n) + 0.3 * hash_unitvar(seed, (256, 256), stream=26 + 4 * n + c)
        wts[n, 0] = 1.0 / (1.0 + np.exp(-6.0 * (0.5 - np.hypot(xx - 0.1 * n, yy + 0.1)))) * (0.8 + 0.2 * hash_uniform(seed, 65536, stream=40 + n).reshape(256, 256))
    return {"fs": fs, "kp_s": kp_s, "kp_d": kp_d, "Rs": Rs, "Rd": Rd, "tgt_head_img": np.clip(img, -1.0, 1.0), "tgt_head_weights": wts.astype(np.float32)}


def torso_appearance_shapes(in_dim=3):
    """[(state_dict key, shape)] of AppearanceFeatureExtractor(in_dim) (modules/real3d/facev2v_warp/network2.py:24-36): 107 entries."""
    bn = lambda p, c: [(p + n, (c,)) for n in ("weight", "bias", "running_mean", "running_var")] + [(p + "num_batches_tracked", ())]
    conv = lambda p, co, ci, *k: [(p + "weight", (co, ci) + k), (p + "bias", (co,))]
    out = conv("in_conv.layers.0.", 64, in_dim, 7, 7) + bn("in_conv.layers.1.", 64)
    for i, (ci, co) in enumerate(((64, 128), (128, 256))):
        out += conv("down.%d.layers.0.layers.0." % i, co, ci, 3, 3) + bn("down.%d.layers.0.layers.1." % i, co)
    out += conv("mid_conv.", TORSO_C * TORSO_D, 256, 1, 1)
    for i in range(6):
        for j in range(2):
            p = "res.%d.layers.%d.layers." % (i, j)
            out += bn(p + "0.", TORSO_C) + conv(p + "2.", TORSO_C, TORSO_C, 3, 3, 3)
    return out


# weight gains of synth_torso_appearance (x 1 / sqrt(fan_in)), chosen so that on synth_torso_appearance_inputs every ReLU zeroes a
# middling share of its inputs and every ResBlock3D's branch and input both carry a good part of its output
# (tests/golden/make_golden_torso_appearance.py asserts all of it on the reference's output)
APPEARANCE_GAINS = {"in_conv": 1.5, "down": 2.0, "mid_conv": 1.5, "res": 1.4}


def synth_torso_appearance(seed, in_dim=3):
    """A full state_dict (numpy) of the appearance feature extractor.  Conv weights ~ N(0, gain^2 / fan_in) with APPEARANCE_GAINS by
    module, biases 0.1 n (0.3 n in front of a BatchNorm); BatchNorm: weight 1 + 0.1 n, bias and running_mean 0.3 n, running_var in
    [0.5, 2]."""
    sd = {}
    shapes = torso_appearance_shapes(in_dim)
    names = dict(shapes)
    for i, (key, shape) in enumerate(shapes):
        st = 5000 + i
        last = key.rsplit(".", 1)[-1]
        if last == "num_batches_tracked":
            v = np.array(0, dtype=np.int64)
        elif last == "running_var":
            v = np.float32(0.5) + np.float32(1.5) * hash_uniform(seed, shape[0], st)
        elif last == "running_mean":
            v = hash_unitvar(seed, shape, st) * np.float32(0.3)
        elif len(shape) == 1 and (key[:-len(last)] + "running_mean") in names:           # BatchNorm weight / bias
            v = hash_unitvar(seed, shape, st) * np.float32(0.3) if last == "bias" else np.float32(1.0) + hash_unitvar(seed, shape, st) * np.float32(0.1)
        elif last == "bias":
            front = key[:-6].rsplit(".", 1)[0] + ".1.running_mean" in names              # a "CNA" conv: its bias meets the BatchNorm's mean
            v = hash_unitvar(seed, shape, st) * np.float32(0.3 if front else 0.1)
        else:
            gain = next(g for p, g in APPEARANCE_GAINS.items() if key.startswith(p))
            v = hash_unitvar(seed, shape, st) * np.float32(gain / math.sqrt(int(np.prod(shape[1:]))))
        sd[key] = np.asarray(v, dtype=np.int64 if last == "num_batches_tracked" else np.float32)
    return sd


def synth_torso_appearance_inputs(seed, N=1, in_dim=3, H=256, W=256):
    """The input of AppearanceFeatureExtractor.forward as WarpBasedTorsoModelMediaPipe.forward builds it (facev2v_warp/model2.py:226-230):
    x [N, in_dim, H, W]: channels 0 .. 2 an image in [-1, 1] (a smooth pattern + noise), any further channels (rgb_alpha: the torso and
    head masks) in [0, 1].  Every sample differs."""
    ly, lx = np.linspace(-1.0, 1.0, H, dtype=np.float32), np.linspace(-1.0, 1.0, W, dtype=np.float32)
    yy, xx = np.meshgrid(ly, lx, indexing="ij")
    x = np.empty((N, in_dim, H, W), np.float32)
    for n in range(N):
        for c in range(in_dim):
            noise = hash_unitvar(seed, (H, W), stream=51 + 8 * n + c)
            if c < 3:
                x[n, c] = np.clip(0.6 * np.sin(3.0 * xx * (c + 1) + 2.0 * yy + n) + 0.3 * noise, -1.0, 1.0)
            else:
                x[n, c] = np.clip(1.0 / (1.0 + np.exp(-6.0 * (0.5 - np.hypot(xx - 0.1 * n, yy + 0.2 * (c - 3))))) + 0.1 * noise, 0.0, 1.0)
    return {"x": x}


def synth_torso_glue_inputs(seed, N=1, Cs=6, Hs=512, Ws=512, C=32, D=16, h=64, w=64):
    """Inputs of the glue of WarpBasedTorsoModelMediaPipe.forward (facev2v_warp/model2.py:231-236): segmap [N, Cs, Hs, Ws] in [0, 1] (per
    class a soft blob + noise, so that the resized pair, their sum and its dilation all vary over the image) and the extractor's volume
    feats [N, C, D, h, w], unit variance.  Every sample differs."""
    ly, lx = np.linspace(-1.0, 1.0, Hs, dtype=np.float32), np.linspace(-1.0, 1.0, Ws, dtype=np.float32)
    yy, xx = np.meshgrid(ly, lx, indexing="ij")
    seg = np.empty((N, Cs, Hs, Ws), np.float32)
    for n in range(N):
        for c in range(Cs):
            cx, cy = 0.8 * hash_uniform(seed, 2, stream=300 + 16 * n + c) - 0.4
            blob = 1.0 / (1.0 + np.exp(-5.0 * (0.45 - np.hypot(xx - cx, yy - cy))))
            seg[n, c] = np.clip(0.6 * blob + 0.12 * hash_unitvar(seed, (Hs, Ws), stream=400 + 16 * n + c), 0.0, 1.0)
    return {"segmap": seg, "feats": hash_unitvar(seed, (N, C, D, h, w), stream=500)}


def synth_torso_onehot_segmap(seed, N=1, Cs=6, Hs=512, Ws=512, centres=10, specks=24, ratio=8, torso=(2, 4)):
    """A one-hot segmap [N, Cs, Hs, Ws] whose label image consists of blobs: the class of the nearest of `centres` points, point i of
    class i % Cs, plus `specks` single pixels of class torso[0] outside the torso classes, on rows and columns that a resize by the even
    integer `ratio` reads (they resize to 1/4, which the dilation then spreads where no blob is near).  At such a ratio every bilinear
    weight is 1/2, so fp32 evaluates the glue of facev2v_warp/model2.py:231-236 exactly."""
    ly, lx = np.linspace(0.0, 1.0, Hs, dtype=np.float32), np.linspace(0.0, 1.0, Ws, dtype=np.float32)
    yy, xx = np.meshgrid(ly, lx, indexing="ij")
    seg = np.zeros((N, Cs, Hs, Ws), np.float32)
    for n in range(N):
        p = hash_uniform(seed, 2 * centres, stream=600 + n).reshape(centres, 2)
        label = np.argmin([np.hypot(xx - px, yy - py) for px, py in p], axis=0) % Cs
        q = hash_uniform(seed, 2 * specks, stream=700 + n).reshape(specks, 2)
        for qy, qx in q:
            y, x = int(qy * Hs) // ratio * ratio + ratio // 2 - 1, int(qx * Ws) // ratio * ratio + ratio // 2 - 1
            if label[y, x] not in torso:
                label[y, x] = torso[0]
        for c in range(Cs):
            seg[n, c] = label == c
    return seg


BFM_FOV_DEG = 2.0 * math.degrees(math.atan(112.0 / 1015.0))     # SECC_Renderer's camera (deep_3drecon/secc_renderer.py:14: centre 112, focal 1015)


def synth_face_mesh(G, seed, C=3):
    """A face-like mesh for the rasteriser (real3dportrait_amd/mesh_renderer.py): a (G + 1)^2 grid over [-1.05, 1.05]^2 with sigma = 0.01
    jitter in x and y and z = 10 - 0.9 cos(1.3 u) cos(1.1 v) + 0.05 noise, split into 2 G^2 triangles, plus a second copy with x and y
    scaled by 0.35 and z - 0.4: a nearer layer, so that the depth test decides pixels.  About 95 % of the image at BFM_FOV_DEG.
    Returns vertex [N, 3] float32 (camera space), tri [M, 3] int64 and feat [N, C] float32 in [0, 1); N = 2 (G + 1)^2, M = 4 G^2."""
    n = (G + 1) * (G + 1)
    lin = np.linspace(-1.05, 1.05, G + 1)
    v, u = np.meshgrid(lin, lin, indexing="ij")
    u, v = u.reshape(-1), v.reshape(-1)
    jit = hash_unitvar(seed, (3, n), stream=40).astype(np.float64)
    x, y = u + 0.01 * jit[0], v + 0.01 * jit[1]
    z = 10.0 - 0.9 * np.cos(1.3 * u) * np.cos(1.1 * v) + 0.05 * jit[2]
    layer = np.stack([x, y, z], axis=1)
    near = np.stack([0.35 * x, 0.35 * y, z - 0.4], axis=1)
    r, c = np.meshgrid(np.arange(G), np.arange(G), indexing="ij")
    i00 = (r * (G + 1) + c).reshape(-1)
    i01, i10, i11 = i00 + 1, i00 + G + 1, i00 + G + 2
    tri = np.concatenate([np.stack([i00, i01, i11], axis=1), np.stack([i00, i11, i10], axis=1)], axis=0).astype(np.int64)
    return {"vertex": np.concatenate([layer, near], axis=0).astype(np.float32), "tri": np.concatenate([tri, tri + n], axis=0),
            "feat": hash_uniform(seed, 2 * n * C, stream=41).reshape(2 * n, C)}


def synth_secc_eyes(H, W, seed, crossing=False, zero_channel=0, right_hole=True):
    """A SECC-like map [3, H, W] float32 in [-1, 1] for the blink edit (real3dportrait_amd/edit_secc.py): an elliptical face
    ((u - .5) / .42)^2 + ((v - .52) / .47)^2 < 1 (u, v the pixel centres in [0, 1]) over a background of -1, smooth colours 2 x - 1 with
    x in [0.02, 1] (a colour never quantises to 0) plus sigma = 0.01 noise, and two elliptical eye holes of -1 at u = 0.37 and 0.63,
    v = 0.385 (the right one 0.013 lower), half-axes 0.065 x 0.028.  crossing: the right hole sits at u = 0.56 with a half-axis of 0.09, so it
    crosses the middle column into the left prior region.  zero_channel = n: n face pixels get one channel at x = 0.001, which quantises
    to 0 (the reference then counts the pixel as non-face).  right_hole=False leaves the right prior region without an eye pixel."""
    v, u = np.meshgrid((np.arange(H) + 0.5) / H, (np.arange(W) + 0.5) / W, indexing="ij")
    face = ((u - 0.5) / 0.42) ** 2 + ((v - 0.52) / 0.47) ** 2 < 1.0
    noise = 0.01 * hash_unitvar(seed, (3, H, W), stream=50).astype(np.float64)
    x = np.stack([0.5 + 0.4 * np.sin(3.1 * u + 0.3 * seed) * np.cos(2.3 * v), 0.5 + 0.4 * np.cos(2.7 * u * v + 0.2 * seed),
                  0.5 + 0.35 * np.sin(4.0 * (u - v)) + 0.1 * v]) + noise
    x = np.clip(x, 0.02, 1.0)
    ru, rw = (0.56, 0.09) if crossing else (0.63, 0.065)
    hole = ((u - 0.37) / 0.065) ** 2 + ((v - 0.385) / 0.028) ** 2 < 1.0
    if right_hole:
        hole |= ((u - ru) / rw) ** 2 + ((v - 0.398) / 0.028) ** 2 < 1.0
    if zero_channel:
        ys, xs = np.nonzero(face & ~hole)
        pick = (hash_uniform(seed, 2 * zero_channel, stream=51).reshape(2, -1) * np.array([[len(ys)], [3]])).astype(np.int64)
        x[pick[1], ys[pick[0]], xs[pick[0]]] = 0.001
    img = 2.0 * x - 1.0
    img[:, ~face | hole] = -1.0
    return img.astype(np.float32)


SECC_EYES = ((0.37, 0.385), (0.63, 0.398))          # (u, v) of synth_secc_eyes' two holes, half-axes 0.065 x 0.028 of the image


def synth_portrait_segmap(H, W, seed, shift=0.0, low_neck=True):
    """A one-hot portrait segmap uint8 [6, H, W] for real3dportrait_amd/source_conditions.py, the segmenter's classes: 0 background,
    1 hair, 2 body skin (the neck), 3 face skin, 4 clothes, 5 others (a glasses strip).  u, v are the pixel centres in [0, 1], the person
    is centred on u = 0.5 + shift.  Clothes lie below a wavy shoulder line v_s(u) that falls away from the neck; the neck is the strip
    |u - c| < 0.085 between the face and the shoulder line; the hair is an ellipse behind the face with two strands (0.17 < |u - c| <
    0.23) that hang down to the shoulder line, so in their columns clothes lie directly under hair; the face is an ellipse over both; the
    glasses a horizontal strip across it.  low_neck: in the columns 0.04 < u < 0.10 a patch of face skin ends 5 rows above the bottom of
    the image and the bottom row is body skin, so the dilated neck of these columns has 4 pixels (the bottom border cuts it) with face
    skin directly above: the only way a column of inpaint_torso_job has a pixel count below 5."""
    v, u = np.meshgrid((np.arange(H) + 0.5) / H, (np.arange(W) + 0.5) / W, indexing="ij")
    c = 0.5 + shift
    du = np.abs(u - c)
    v_s = 0.74 + 0.025 * np.sin(2 * np.pi * 2.5 * u + 0.7 * seed) + 0.5 * np.maximum(du - 0.12, 0.0)
    label = np.zeros((H, W), np.int64)
    label[(v > v_s) & (du < 0.46)] = 4
    label[(du < 0.085) & (v > 0.45) & (v <= v_s)] = 2
    label[((u - c) / 0.25) ** 2 + ((v - 0.33) / 0.25) ** 2 < 1.0] = 1
    label[(du > 0.17) & (du < 0.23) & (v > 0.33) & (v <= v_s)] = 1
    label[((u - c) / 0.17) ** 2 + ((v - 0.40) / 0.20) ** 2 < 1.0] = 3
    label[(np.abs(v - 0.37) < 0.018) & (du < 0.14)] = 5
    if low_neck:
        cols = (u[0] > 0.04) & (u[0] < 0.10)
        label[H - 12:H - 4, cols] = 3
        label[H - 1, cols] = 2
    return (label[None] == np.arange(6)[:, None, None]).astype(np.uint8)


def synth_portrait_image(H, W, seed, shift=0.0):
    """The image uint8 [H, W, 3] that goes with synth_portrait_segmap: smooth colours that move with the person plus per-pixel noise, so
    that no two neighbouring pixels are likely to agree in all three channels."""
    v, u = np.meshgrid((np.arange(H) + 0.5) / H, (np.arange(W) + 0.5) / W, indexing="ij")
    u = u - shift
    noise = hash_unitvar(seed, (3, H, W), stream=60).astype(np.float64)
    x = np.stack([0.5 + 0.3 * np.sin(5.1 * u + 0.3 * seed) * np.cos(3.3 * v), 0.5 + 0.3 * np.cos(6.7 * u * v + 0.2 * seed),
                  0.5 + 0.25 * np.sin(7.0 * (u - v)) + 0.1 * v]) + 0.08 * noise
    return np.ascontiguousarray(np.clip(x * 255.0, 0.0, 255.0).astype(np.uint8).transpose(1, 2, 0))


def synth_face_model(G, seed, Ki=80, Ke=64):
    """A morphable face model for real3dportrait_amd/face_model.py and driving_motion.py, with the attributes the reference's
    ParametricFaceModel, SECC_Renderer and Face3DHelper carry (BFM data exists on no machine this project is built on):

        mean_shape [3 N, 1]   a single-layer (G + 1)^2 grid like synth_face_mesh's: x, y over [-1.05, 1.05]^2 with a jitter of sigma = a tenth of a cell, model
                              z = 0.9 cos(1.3 u) cos(1.1 v), so that camera z = camera_distance - z = 10 - 0.9 cos cos
        id_base [3 N, Ki], exp_base [3 N, Ke]   smooth displacement fields of amplitude 0.004 per unit coefficient: column k is
                              sin(a_k u + p_k) sin(b_k v + q_k) times a fixed unit direction d_k, a_k, b_k in [0.5, 3): the gradient of a
                              unit-variance sum of all columns stays near 0.05, so no triangle flips
        tri [M, 3] int64      2 G^2 triangles minus those whose centre projects (mean shape, BFM_FOV_DEG, x negated as the renderer does)
                              into one of two ellipses at SECC_EYES, as SECC_Renderer removes the eye faces; the blink edit accepts the
                              rendered map.  Face 0 is the zero-area triangle (0, 0, 0): the reference's mask, pix_to_face > 0, turns face 0
                              of the FIRST mesh of every batch into background, and with a face that covers nothing a map cannot depend on
                              where its frame falls in a chunk
        feat [N, 3]           in [0.02, 1]: a colour never quantises to 0
        keypoints [68] int64, key_mean_shape [68, 3], key_id_base [204, Ki], key_exp_base [204, Ke]   as Face3DHelper.load_3dmm cuts them
        camera_distance 10.0

    float32 throughout, every number from hash_*: the same (G, seed, Ki, Ke) gives the same model everywhere."""
    n = (G + 1) * (G + 1)
    lin = np.linspace(-1.05, 1.05, G + 1)
    v, u = np.meshgrid(lin, lin, indexing="ij")
    u, v = u.reshape(-1), v.reshape(-1)
    jit = hash_unitvar(seed, (2, n), stream=70).astype(np.float64)
    sigma = 0.1 * 2.1 / G                    # |jitter| <= 3.47 sigma: two neighbours never cross
    x, y, z = u + sigma * jit[0], v + sigma * jit[1], 0.9 * np.cos(1.3 * u) * np.cos(1.1 * v)
    mean = np.stack([x, y, z], axis=1)

    def basis(K, stream):
        if K == 0:
            return np.zeros((3 * n, 0), np.float32)
        par = hash_uniform(seed, 4 * K, stream).reshape(4, K).astype(np.float64)
        d = hash_unitvar(seed, (K, 3), stream + 1).astype(np.float64) + 1e-3
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        a, b, p, q = 0.5 + 2.5 * par[0], 0.5 + 2.5 * par[1], 2 * math.pi * par[2], 2 * math.pi * par[3]
        field = np.sin(u[:, None] * a + p) * np.sin(v[:, None] * b + q)                    # [n, K]
        return (0.004 * field[:, None, :] * d.T[None]).reshape(3 * n, K).astype(np.float32)

    r, c = np.meshgrid(np.arange(G), np.arange(G), indexing="ij")
    i00 = (r * (G + 1) + c).reshape(-1)
    i01, i10, i11 = i00 + 1, i00 + G + 1, i00 + G + 2
    tri = np.concatenate([np.stack([i00, i01, i11], axis=1), np.stack([i00, i11, i10], axis=1)], axis=0).astype(np.int64)
    centre = mean[tri].mean(axis=1)
    s = 1015.0 / 112.0                                                                    # 1 / tan(BFM_FOV_DEG / 2)
    cz = 10.0 - centre[:, 2]
    pu, pv = 0.5 * (1.0 + s * centre[:, 0] / cz), 0.5 * (1.0 - s * centre[:, 1] / cz)      # x_ndc = s (-x) / z = 1 - 2 u; y_ndc = 1 - 2 v
    eye = np.zeros(len(tri), bool)
    for eu, ev in SECC_EYES:
        eye |= ((pu - eu) / 0.065) ** 2 + ((pv - ev) / 0.028) ** 2 < 1.0
    tri = np.concatenate([np.zeros((1, 3), np.int64), tri[~eye]], axis=0)
    key = (np.arange(68) * n) // 68 + (hash_uniform(seed, 68, stream=75) * (n // 68)).astype(np.int64)
    id_base, exp_base = basis(Ki, 71), basis(Ke, 73)
    mean32 = mean.astype(np.float32)
    return {"mean_shape": mean32.reshape(-1, 1), "id_base": id_base, "exp_base": exp_base, "tri": tri,
            "feat": (0.02 + 0.98 * hash_uniform(seed, 3 * n, stream=76).reshape(n, 3)).astype(np.float32), "keypoints": key,
            "key_mean_shape": mean32[key], "key_id_base": id_base.reshape(n, 3, Ki)[key].reshape(3 * 68, Ki),
            "key_exp_base": exp_base.reshape(n, 3, Ke)[key].reshape(3 * 68, Ke), "camera_distance": 10.0}


MP468_UNMATCHED = (93, 127, 132, 234, 323, 356, 361, 454)          # unmatch_mask of fit_3dmm_landmark.py: mediapipe points without a mesh vertex


def synth_face_keys(model, L, seed):
    """L key rows of a synth_face_model for the landmark fit (real3dportrait_amd/fit_3dmm.py), as ParametricFaceModel cuts them with
    keypoint_mode='mediapipe' (bfm.py:60-63, 80-82): one vertex per point, drawn by the project's hash from the point's stretch of the mesh (distinct vertices, as landmarks are), and the MP468_UNMATCHED indices below L
    mapped to vertex 0 as the reference maps its negative entries.  Returns keypoints [L] int64, key_mean_shape [L, 3], key_id_base
    [3 L, Ki] and key_exp_base [3 L, Ke]; `model` itself is not changed."""
    n = model["mean_shape"].size // 3
    Ki, Ke = model["id_base"].shape[1], model["exp_base"].shape[1]
    lo = (np.arange(L + 1, dtype=np.int64) * n) // L          # point i draws from vertices lo[i] .. lo[i + 1]: distinct while L <= n, and spread
    key = np.minimum(lo[:-1] + (hash_uniform(seed, L, stream=77).astype(np.float64) * np.maximum(lo[1:] - lo[:-1], 1)).astype(np.int64), n - 1)
    key[[i for i in MP468_UNMATCHED if i < L]] = 0
    return {"keypoints": key, "key_mean_shape": model["mean_shape"].reshape(n, 3)[key],
            "key_id_base": model["id_base"].reshape(n, 3, Ki)[key].reshape(3 * L, Ki),
            "key_exp_base": model["exp_base"].reshape(n, 3, Ke)[key].reshape(3 * L, Ke)}


AUDIO2MOTION_HPARAMS = {"use_mouth_amp_embed": True, "use_eye_amp_embed": False}          # egs/os_avatar/audio2motion_vae.yaml


def audio2motion_shapes(pitch=True, audio_in_dim=1024):
    """{state_dict key: shape} of PitchContourVAEModel(AUDIO2MOTION_HPARAMS) / VAEModel (modules/audio2motion/vae.py:272-454), in
    state_dict order, read off this package's classes (tests compare the names with the recorded reference's)."""
    from . import audio2motion as a
    m = a.PitchContourVAEModel(AUDIO2MOTION_HPARAMS, audio_in_dim=audio_in_dim) if pitch else a.VAEModel(audio_in_dim=audio_in_dim)
    return {k: tuple(v.shape) for k, v in m.state_dict().items()}


def synth_audio2motion(seed, pitch=True, audio_in_dim=1024):
    """A state_dict (numpy) for the audio-to-motion VAE at which a passing comparison means something: every convolution keeps its input's
    scale (sigma = gain / sqrt(fan in)), so the gates stay unsaturated; weight_g is ||v|| times 1.25 .. 1.5, never the ||v|| a missing
    gain would give; the flows' post layers, which the reference initialises to zero, are not zero; the BatchNorm statistics are not
    (0, 1) and its affine part is not (1, 0).  Every number from hash_*: the same arguments give the same model everywhere."""
    shapes = audio2motion_shapes(pitch, audio_in_dim)
    sd = {}
    for n, (key, shape) in enumerate(shapes.items()):
        st = 1000 + 2 * n
        leaf = key.rsplit(".", 1)[-1]
        if leaf == "num_batches_tracked":
            sd[key] = np.array(1, np.int64)
        elif leaf == "running_var":
            sd[key] = (0.5 + hash_uniform(seed, shape[0], st)).astype(np.float32)
        elif leaf == "running_mean":
            sd[key] = (0.3 * hash_unitvar(seed, shape, st)).astype(np.float32)
        elif leaf == "weight_g":
            sd[key] = (1.25 + 0.25 * hash_uniform(seed, shape[0], st)).reshape(shape).astype(np.float32)          # x ||v|| below
        elif len(shape) == 1 and leaf == "weight":                       # BatchNorm1d's
            sd[key] = (1.0 + 0.3 * hash_unitvar(seed, shape, st)).astype(np.float32)
        elif len(shape) == 1 and leaf in ("mouth_amp_embed", "eye_amp_embed"):
            sd[key] = hash_unitvar(seed, shape, st)
        elif len(shape) == 1:                                            # biases
            sd[key] = (0.1 * hash_unitvar(seed, shape, st)).astype(np.float32)
        elif "embed" in key:                                             # blink_embed, pitch_embed
            sd[key] = hash_unitvar(seed, shape, st)
        else:
            # Conv1d [cout, cin, k], Linear [cout, cin]: fan in cin k; ConvTranspose1d(16, 256, 4, 4) [cin, cout, k]: one tap reaches an output row
            fan = shape[0] if "decoder.pre_net" in key else int(np.prod(shape[1:]))
            gain = 0.7 if leaf == "weight_v" else (2.0 if key.endswith("post.weight") else 1.0)
            sd[key] = (hash_unitvar(seed, shape, st) * np.float32(gain / math.sqrt(fan))).astype(np.float32)
    for key in shapes:
        if key.endswith("weight_g"):
            v = sd[key[:-1] + "v"].astype(np.float64)
            sd[key] = (sd[key] * np.sqrt((v * v).sum(axis=(1, 2), keepdims=True))).astype(np.float32)
    return sd


def synth_audio2motion_inputs(seed, B, T):
    """One batch for the audio-to-motion VAE: audio [B, 2 T, 1024] of unit variance, f0 [B, 2 T] in Hz, blink [B, 2 T, 1] int64, mouth_amp
    [B, 1], y_mask [B, T]; sample b differs from sample 0 in all of them.  f0: a slow contour between 80 and 400 Hz; the frames 4 n + 2
    (at least three, and every one of a short clip's tail) are unvoiced, f0 = 0; a voiced frame whose f0_to_coarse value + 0.5 (in fp64)
    lies within 2e-3 of an integer is moved up in steps of 0.37 Hz until it does not, so that no fp32 log can move an index.  blink: ones
    on the frames [T / 2, T / 2 + 3) of sample 0, every fifth frame of the others.  y_mask: ones, and zeros on the last max(1, T / 4)
    rows of every sample but the first."""
    audio = hash_unitvar(seed, (B, 2 * T, 1024), stream=1)
    ph = hash_uniform(seed, 3 * B, stream=2).reshape(B, 3).astype(np.float64)
    t = np.arange(2 * T, dtype=np.float64)[None]
    f0 = 240.0 + 160.0 * np.sin(2 * math.pi * (ph[:, :1] + t * (0.013 + 0.01 * ph[:, 1:2]))) * np.cos(0.05 * t + ph[:, 2:3])
    f0 += 3.0 * hash_unitvar(seed, (B, 2 * T), stream=3)
    f0 = np.clip(f0, 80.0, 400.0).astype(np.float32)
    lo, hi = 1127 * math.log(1 + 50.0 / 700), 1127 * math.log(1 + 1100.0 / 700)
    for _ in range(64):
        m = (1127 * np.log(1 + f0.astype(np.float64) / 700) - lo) * 254 / (hi - lo) + 1 + 0.5
        near = np.abs(m - np.rint(m)) < 2e-3
        if not near.any():
            break
        f0 = np.where(near, f0 + np.float32(0.37), f0).astype(np.float32)
    f0[:, 2::4] = 0.0
    if T < 6:
        f0[:, 2:] = 0.0
    blink = np.zeros((B, 2 * T, 1), np.int64)
    blink[0, T // 2:T // 2 + 3] = 1
    blink[1:, ::5] = 1
    mask = np.ones((B, T), np.float32)
    mask[1:, T - max(1, T // 4):] = 0.0
    amp = (0.25 + 0.5 * hash_uniform(seed, B, stream=4)).reshape(B, 1).astype(np.float32)
    return {"audio": audio, "f0": f0, "blink": blink, "mouth_amp": amp, "y_mask": mask}


# HuBERT-large (facebook/hubert-large-ls960-ft), the structure real3dportrait_amd/hubert.py builds; a config overrides any of these
HUBERT_LARGE = {"hidden_size": 1024, "num_hidden_layers": 24, "num_attention_heads": 16, "intermediate_size": 4096, "conv_dim": (512,) * 7,
                "conv_kernel": (10, 3, 3, 3, 3, 2, 2), "conv_stride": (5, 2, 2, 2, 2, 2, 2), "num_conv_pos_embeddings": 128,
                "num_conv_pos_embedding_groups": 16, "layer_norm_eps": 1e-5}


def hubert_shapes(cfg=None, masked_spec_embed=True):
    """[(state_dict key, shape)] of transformers.HubertModel with the large model's structure (layer-norm feature extractor, stable layer
    norm, a weight-norm positional conv held as parametrizations.weight.original0 / original1) for the widths of cfg over HUBERT_LARGE."""
    c = dict(HUBERT_LARGE, **(cfg or {}))
    H, I = c["hidden_size"], c["intermediate_size"]
    lin = lambda p, co, ci: [(p + ".weight", (co, ci)), (p + ".bias", (co,))]
    norm = lambda p, n: [(p + ".weight", (n,)), (p + ".bias", (n,))]
    out = [("masked_spec_embed", (H,))] if masked_spec_embed else []
    cin = 1
    for i, (co, k) in enumerate(zip(c["conv_dim"], c["conv_kernel"])):
        p = "feature_extractor.conv_layers.%d." % i
        out += [(p + "conv.weight", (co, cin, k)), (p + "conv.bias", (co,))] + norm(p + "layer_norm", co)
        cin = co
    out += norm("feature_projection.layer_norm", cin) + lin("feature_projection.projection", H, cin)
    kp, gp = c["num_conv_pos_embeddings"], c["num_conv_pos_embedding_groups"]
    p = "encoder.pos_conv_embed.conv."
    out += [(p + "bias", (H,)), (p + "parametrizations.weight.original0", (1, 1, kp)), (p + "parametrizations.weight.original1", (H, H // gp, kp))]
    out += norm("encoder.layer_norm", H)
    for i in range(c["num_hidden_layers"]):
        p = "encoder.layers.%d." % i
        for n in ("k_proj", "v_proj", "q_proj", "out_proj"):
            out += lin(p + "attention." + n, H, H)
        out += norm(p + "layer_norm", H) + lin(p + "feed_forward.intermediate_dense", I, H) + lin(p + "feed_forward.output_dense", H, I)
        out += norm(p + "final_layer_norm", H)
    return out


def synth_hubert(seed, cfg=None, qk_gain=2.0, masked_spec_embed=True):
    """A state_dict (numpy) for hubert_shapes: weights ~ N(0, 1 / fan_in) (2 / fan_in in front of a GELU), the q and k projections times
    qk_gain, biases 0.1 n, LayerNorm weights 1 + 0.1 n, the weight-norm gain g = |n| + 0.5, masked_spec_embed uniform."""
    sd = {}
    for i, (key, shape) in enumerate(hubert_shapes(cfg, masked_spec_embed)):
        st = 7000 + i
        if key == "masked_spec_embed":
            v = hash_uniform(seed, shape[0], st)
        elif key.endswith("original0"):
            v = np.abs(hash_unitvar(seed, shape, st)) + np.float32(0.5)
        elif key.endswith(".bias"):
            v = hash_unitvar(seed, shape, st) * np.float32(0.1)
        elif len(shape) == 1:
            v = np.float32(1.0) + hash_unitvar(seed, shape, st) * np.float32(0.1)
        else:
            gelu_fed = "conv" in key or "intermediate_dense" in key
            v = hash_unitvar(seed, shape, st) * np.float32(math.sqrt((2.0 if gelu_fed else 1.0) / int(np.prod(shape[1:]))))
            if "q_proj" in key or "k_proj" in key:
                v = v * np.float32(qk_gain)
        sd[key] = np.asarray(v, dtype=np.float32)
    return sd
