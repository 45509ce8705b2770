"""The per-frame first half of the face-vid2vid torso network on the HIP torso kernels (r3d_torso_conv3d and r3d_torso_motion_* of
include/r3d_hip.h):

    MotionFieldEstimator  modules/real3d/facev2v_warp/network2.py:162-244 (version v2: with the target-head branch): compress, the
                          heatmaps and the sparse motions, the Conv3d hourglass, tgt_head_encoder, tgt_head_fuser, mask_conv, the
                          mask-weighted deformation and the two occlusion maps

in exact fp32 by default (precision='f32'), or with precision='bf16x3' with every convolution on the split-precision tier of
torso_precision.py (the motion input, the deformation, the resizes and the folds are the same).  It keeps the reference's attribute
names and its 129 state_dict keys, so a reference checkpoint loads with strict=True.
INFERENCE ONLY (eval semantics: BatchNorm on its running statistics); inputs are detached and no autograd graph is built.  The BatchNorms
are folded into the conv weights, biases and prologue vectors in fp64 once per parameter version (_prepare), where the channel groups
are also padded to multiples of 4 and the occlusion weights permuted to the kernel's full-depth form.  The building blocks, the two
BatchNorm folds, the module base (_prepare, work buffers, from_reference) and the launch wrappers are torso_layers.py's.
"""
import torch
import torch.nn as nn

from . import _lib
from .torso_layers import (LEAKY, SIGMOID, _check_f32, _conv, _conv3d, _ConvBlock, _kernel_weight3d, _pad4, _ResBlock, _TorsoModule, conv_layer,
                           conv_weight64, fold_cna, fold_res_pair)
from .torso_precision import F32

DEPTH, GRID, HEAD, HID = 16, 64, 256, 32          # the feature volume [N, C, 16, 64, 64], the head image 256^2, tgt_head_hid_dim


class _DownBlock3D(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.layers = nn.Sequential(_ConvBlock(3, "CNA", cin, cout, 3), nn.AvgPool3d((1, 2, 2)))


class _UpBlock3D(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.layers = nn.Sequential(nn.Upsample(scale_factor=(1, 2, 2)), _ConvBlock(3, "CNA", cin, cout, 3))


def fold_motion(m, dtype=torch.float32):
    """The estimator's convolutions as kernel calls, folded in fp64 and rounded once to `dtype` (float64: the fold itself, for the tests).
    A dict:  compress (w [4, C], b);  enc: tgt_head_encoder as seven r3d_torso_conv layers in fold_generator's format;  down / up: five
    r3d_torso_conv3d layers each (w [Cout, 3, 3, 3, Cin'], b; the BatchNorm is in the rows and the bias, ReLU and the pool / up-sampling are
    the kernel's);  fuser, mask (k 7);  occ: occlusion_conv and occlusion_conv2 as one full-depth layer with two output channels."""
    f = lambda v: None if v is None else v.to(dtype).contiguous()
    d64 = lambda p: p.detach().double()
    K = m.num_keypoints
    cm = 5 * (K + 1)
    F = {"compress": {"w": f(d64(m.compress.weight).reshape(4, -1)), "b": f(d64(m.compress.bias))}, "enc": [], "down": [], "up": []}

    F["enc"].append(conv_layer(*fold_cna(m.tgt_head_encoder[0], conv_weight64), 7, dtype, act=LEAKY))
    for blk in list(m.tgt_head_encoder)[1:]:
        (w1, b1, ps, pt), (w2, b2) = fold_res_pair(blk.layers[0], blk.layers[1], conv_weight64)
        F["enc"] += [conv_layer(w1, b1, 3, dtype, ps=ps, pt=pt, act=LEAKY), conv_layer(w2, b2, 3, dtype, res=True)]
    for name, seq, pos in (("down", m.down, 0), ("up", m.up, 1)):
        for blk in seq:
            w, b = fold_cna(blk.layers[pos], conv_weight64)
            F[name].append({"w": _kernel_weight3d(w, dtype), "b": f(b)})
    F["fuser"] = {"w": _kernel_weight3d(d64(m.tgt_head_fuser.weight), dtype, [cm, HID, HID]), "b": f(d64(m.tgt_head_fuser.bias))}
    F["mask"] = {"w": _kernel_weight3d(d64(m.mask_conv.weight), dtype), "b": f(d64(m.mask_conv.bias))}
    # Conv2d over x.view(N, 32 D, H, W), channel c D + d  ->  [2, D, 7, 7, 32]
    ow = torch.cat([d64(c.weight).reshape(1, HID, DEPTH, 7, 7) for c in (m.occlusion_conv, m.occlusion_conv2)], dim=0)
    F["occ"] = {"w": _kernel_weight3d(ow, dtype), "b": f(torch.cat([d64(m.occlusion_conv.bias), d64(m.occlusion_conv2.bias)]))}
    return F


def jacobian(Rs, Rd):
    """J = Rs Rd^-1 [N, 3, 3] in elementwise torch ops (the inverse by cross products of Rd's rows): no LAPACK call, no host
    synchronisation, and a sample's J does not depend on the batch it is in."""
    r0, r1, r2 = Rd[:, 0], Rd[:, 1], Rd[:, 2]
    c0, c1, c2 = torch.linalg.cross(r1, r2), torch.linalg.cross(r2, r0), torch.linalg.cross(r0, r1)
    inv = torch.stack([c0, c1, c2], dim=-1) / (r0 * c0).sum(-1)[:, None, None]
    return (Rs[:, :, :, None] * inv[:, None, :, :]).sum(dim=2).contiguous()


class MotionFieldEstimator(_TorsoModule):
    """network2.py:162-244.  forward(fs [N, C, 16, 64, 64], kp_s [N, K, 3], kp_d [N, K, 3], Rs [N, 3, 3], Rd [N, 3, 3], tgt_head_img
    [N, 3, 256, 256], tgt_head_weights [N, 1, 256, 256]) -> (deformation [N, 16, 64, 64, 3], occlusion [N, 1, 64, 64], occlusion_2
    [N, 1, 64, 64]).  The reference fixes these sizes (its resizes to 128^2 and 64^2, :220-222); others raise ValueError."""

    def __init__(self, model_scale="standard", input_channels=34, num_keypoints=4, predict_multiref_occ=True, precision=F32):
        super().__init__(precision)
        if model_scale not in ("standard", "large") or not predict_multiref_occ:
            raise NotImplementedError("MotionFieldEstimator: only model_scale 'standard' with predict_multiref_occ has a HIP implementation "
                                      "(network2.py:177-183,232-236; got %r, predict_multiref_occ=%r)" % (model_scale, predict_multiref_occ))
        K = num_keypoints
        down, up = [5 * (K + 1), 64, 128, 256, 512, 1024], [1024, 512, 256, 128, 64, 32]
        self.input_channels, self.num_keypoints, self.predict_multiref_occ = input_channels, K, True
        self.compress = nn.Conv3d(input_channels, 4, 1, 1, 0)
        self.down = nn.Sequential(*[_DownBlock3D(down[i], down[i + 1]) for i in range(5)])
        self.up = nn.Sequential(*[_UpBlock3D(up[i], up[i + 1]) for i in range(5)])
        self.tgt_head_encoder = nn.Sequential(_ConvBlock(2, "CNA", 4, HID, 7), *[_ResBlock(2, HID) for _ in range(3)])
        self.tgt_head_fuser = nn.Conv3d(HID + down[0] + up[-1], HID, 7, 1, 3)
        self.mask_conv = nn.Conv3d(HID, K + 1, 7, 1, 3)
        self.occlusion_conv = nn.Conv2d(HID * DEPTH, 1, 7, 1, 3)
        self.occlusion_conv2 = nn.Conv2d(HID * DEPTH, 1, 7, 1, 3)
        self.C, self.D = down[0] + up[-1], DEPTH

    def _fold(self):
        return fold_motion(self)

    def _new_buffers(self, dev, N):
        e = lambda *n: torch.empty(*n, device=dev, dtype=torch.float32)
        cp = _pad4(5 * (self.num_keypoints + 1))
        vox = N * DEPTH * GRID * GRID
        return {"fs": e(vox * self.input_channels), "inp": e(vox * cp), "fuse": e(vox * (cp + 2 * HID)),
                "down": [e(N * DEPTH * (GRID >> (i + 1)) ** 2 * c) for i, c in enumerate((64, 128, 256, 512, 1024))],
                "up": [e(N * DEPTH * (4 << i) ** 2 * c) for i, c in enumerate((512, 256, 128, 64))],
                "head": e(N, 4, 128, 128), "e0": e(N * 128 * 128 * HID), "e1": e(N * 128 * 128 * HID), "feats": e(N, HID, 128, 128),
                "feats64": e(N, HID, GRID, GRID), "x": e(vox * HID), "mask": e(vox * (self.num_keypoints + 1))}

    @torch.no_grad()
    def forward(self, fs, kp_s, kp_d, Rs, Rd, tgt_head_img, tgt_head_weights):
        return self._run(fs, False, kp_s, kp_d, Rs, Rd, None, tgt_head_img, tgt_head_weights)

    @torch.no_grad()
    def forward_cl(self, fs_cl, kp_s, kp_d, Rs, Rd, tgt_head_img, tgt_head_weights, J=None):
        """forward with the volume already channel-last, fs_cl [N, 16, 64, 64, C] (what r3d_torso_volume_to_cl makes of forward's fs, for
        instance r3d_torso_mask_volume's motion_cl): r3d_torso_volume_to_cl is skipped, everything after it is forward's.  J [N, 3, 3]:
        jacobian(Rs, Rd) if the caller holds it already (Rs and Rd may then be None)."""
        return self._run(fs_cl, True, kp_s, kp_d, Rs, Rd, J, tgt_head_img, tgt_head_weights)

    def _run(self, fs, channel_last, kp_s, kp_d, Rs, Rd, J, tgt_head_img, tgt_head_weights):
        K, C, D, S = self.num_keypoints, self.input_channels, DEPTH, GRID
        fs = _check_f32(fs, "fs", 5)
        N = fs.shape[0]
        img, wts = _check_f32(tgt_head_img, "tgt_head_img", 4), _check_f32(tgt_head_weights, "tgt_head_weights", 4)
        kp_s, kp_d = _check_f32(kp_s, "kp_s", 3), _check_f32(kp_d, "kp_d", 3)
        want = (N, D, S, S, C) if channel_last else (N, C, D, S, S)
        if tuple(fs.shape) != want or tuple(img.shape) != (N, 3, HEAD, HEAD) or tuple(wts.shape) != (N, 1, HEAD, HEAD):
            raise ValueError("MotionFieldEstimator: expected fs %s, tgt_head_img [N, 3, %d, %d] and tgt_head_weights "
                             "[N, 1, %d, %d] (network2.py:220-222), got %s, %s and %s"
                             % (("[N, %d, %d, %d, %d]" % want[1:]), HEAD, HEAD, HEAD, HEAD, tuple(fs.shape), tuple(img.shape), tuple(wts.shape)))
        if J is None:
            Rs, Rd = _check_f32(Rs, "Rs", 3), _check_f32(Rd, "Rd", 3)
            if tuple(Rs.shape) != (N, 3, 3) or tuple(Rd.shape) != (N, 3, 3):
                raise ValueError("MotionFieldEstimator: expected Rs, Rd [N, 3, 3], got %s and %s" % (tuple(Rs.shape), tuple(Rd.shape)))
            J = jacobian(Rs, Rd)
        else:
            J = _check_f32(J, "J", 3)
            if tuple(J.shape) != (N, 3, 3):
                raise ValueError("MotionFieldEstimator: expected J [N, 3, 3], got %s" % (tuple(J.shape),))
        if tuple(kp_s.shape) != (N, K, 3) or tuple(kp_d.shape) != (N, K, 3):
            raise ValueError("MotionFieldEstimator: expected kp_s, kp_d [N, %d, 3], got %s and %s" % (K, tuple(kp_s.shape), tuple(kp_d.shape)))
        dev = fs.device
        F, w = self._prepare(), self._buffers_for(dev, N)
        st = torch.cuda.current_stream().cuda_stream
        cp, pr = _pad4(5 * (K + 1)), self.precision
        fcs = cp + 2 * HID
        # the hourglass input, also the first channel group of the fuser's input
        fs_cl = fs
        if not channel_last:
            fs_cl = w["fs"]
            _lib.call("r3d_torso_volume_to_cl", fs, N, C, D, S, S, fs_cl, st)
        _lib.call("r3d_torso_motion_input", fs_cl, N, C, D, S, S, F["compress"]["w"], F["compress"]["b"], kp_s, kp_d, J, K, w["inp"], cp, w["fuse"],
                  fcs, st)
        # the hourglass; its last conv writes the second group
        x, cin, size = w["inp"], cp, S
        for i, L in enumerate(F["down"]):
            _conv3d(x, N, D, size, size, cin, L, 3, w["down"][i], act=LEAKY, pool=1, precision=pr)
            x, cin, size = w["down"][i], L["w"].shape[0], size // 2
        for i, L in enumerate(F["up"]):
            last = i == 4
            _conv3d(x, N, D, size, size, cin, L, 3, w["fuse"] if last else w["up"][i], ycs=fcs if last else None, yco=cp if last else 0,
                    up=1, act=LEAKY, precision=pr)
            x, cin, size = (None if last else w["up"][i]), L["w"].shape[0], size * 2
        # the head branch: 256^2 -> 128^2, tgt_head_encoder, -> 64^2, repeated over depth into the third group
        head_in = torch.cat([img, wts], dim=1)
        _lib.call("r3d_resize_bilinear", head_in, N * 4, HEAD, HEAD, w["head"], 128, 128, 0, st)
        E = F["enc"]
        _conv(w["head"], N, 128, 128, 4, E[0], y=w["e0"], in_nchw=True, precision=pr)
        for i in range(3):
            _conv(w["e0"], N, 128, 128, HID, E[1 + 2 * i], y=w["e1"], precision=pr)
            if i < 2:
                _conv(w["e1"], N, 128, 128, HID, E[2 + 2 * i], y=w["e0"], res=w["e0"], precision=pr)
            else:
                _conv(w["e1"], N, 128, 128, HID, E[2 + 2 * i], y_nchw=w["feats"], res=w["e0"], precision=pr)
        _lib.call("r3d_resize_bilinear", w["feats"], N * HID, 128, 128, w["feats64"], S, S, 0, st)
        _lib.call("r3d_torso_motion_broadcast", w["feats64"], N, HID, S, S, D, w["fuse"], fcs, cp + HID, st)
        # fuser, mask, deformation, occlusions
        _conv3d(w["fuse"], N, D, S, S, fcs, F["fuser"], 7, w["x"], precision=pr)
        _conv3d(w["x"], N, D, S, S, HID, F["mask"], 7, w["mask"], precision=pr)
        deformation = torch.empty(N, D, S, S, 3, device=dev, dtype=torch.float32)
        _lib.call("r3d_torso_motion_deform", w["mask"], N, D, S, S, K, kp_s, kp_d, J, deformation, st)
        occ = torch.empty(N, 2, S, S, device=dev, dtype=torch.float32)
        _conv3d(w["x"], N, D, S, S, HID, F["occ"], 7, None, act=SIGMOID, full_depth=1, y_ncdhw=occ, precision=pr)
        return deformation, occ[:, 0:1].contiguous(), occ[:, 1:2].contiguous()

    @staticmethod
    def _reference_args(ref):          # a constructed reference MotionFieldEstimator at standard scale
        return {"input_channels": ref.compress.in_channels, "num_keypoints": ref.mask_conv.out_channels - 1}


def is_reference_motion_estimator(m):
    """The reference's v2 MotionFieldEstimator (network2.py: with tgt_head_encoder; network.py's v1 has no target-head branch) at standard
    scale with both occlusion maps."""
    try:
        return (type(m).__name__ == "MotionFieldEstimator" and not type(m).__module__.startswith("real3dportrait_amd")
                and hasattr(m, "tgt_head_encoder") and hasattr(m, "tgt_head_fuser") and len(m.down) == 5 and len(m.up) == 5
                and m.down[0].layers[0].layers[0].out_channels == 64 and m.up[4].layers[1].layers[0].out_channels == 32
                and m.compress.out_channels == 4 and bool(getattr(m, "predict_multiref_occ", False)))
    except (AttributeError, IndexError, TypeError):
        return False
