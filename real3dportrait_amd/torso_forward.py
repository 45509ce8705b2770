"""WarpBasedTorsoModelMediaPipe.forward (modules/real3d/facev2v_warp/model2.py:222-287) over the three HIP torso modules, with what joins
them in the reference in two HIP launches and the appearance volume channel-last from end to end (r3d_torso_seg_input and
r3d_torso_mask_volume of include/r3d_hip.h):

    seg_input     :226-228  cat(img, resize(segmap[:, [2, 4]])): in_conv's input in rgb_alpha mode
    extractor     :230      AppearanceFeatureExtractor.forward_cl: no NCDHW store
    mask_volume   :231-236  the 64 x 64 resize, the mask sum, dilate, the multiply and the concatenation for the estimator, written as the
                            two channel-last volumes the next two modules read
    estimator     :250      MotionFieldEstimator.forward_cl: no r3d_torso_volume_to_cl; the rotations are identities (:248-249), so their
                            Jacobian is a constant of (device, N)
    generator     :260      Generator.forward_cl: straight to r3d_torso_warp, no _VOLUME_CL
    predictor     :262      occlusion_2_predictor on torch's cat([hid, interpolate(occlusion_2)])
    losses        :264-279  in torch, as the reference

patch_model(model, torso_appearance=True, torso_motion=True, torso_generator=True, torso_forward=True) binds `forward` below on the
torso model.  Every call computes everything: nothing is kept from one call to the next but work buffers and that constant.
Still torch: the key-point index select (:238-243), cat([tgt_head_img, tgt_head_weights]) inside the estimator, the interpolate + cat in
front of the predictor, and the losses.  The three gradient-scaling lines (:251-257, x 0.1 + x.detach() 0.9) are the identity in value up
to one rounding and are not evaluated: INFERENCE ONLY, inputs are detached and no autograd graph is built.  What the modules share is
torso_layers.py; this file uses the three through their public forward_cl only.
"""
import torch
import torch.nn.functional as F

from . import _lib
from ._state import StreamBuffers
from .torso_appearance import LAUNCHES as EXTRACTOR_LAUNCHES
from .torso_layers import _check_f32
from .torso_motion import jacobian

SEG_CHANNELS = (2, 4)          # model2.py:227,231: the torso classes of the segmap (tasks/eg3ds/loss_utils/segment_loss/mp_segmenter.py)
KP_INDEX = {4: [0, 8, 16, 27], 9: [0, 3, 6, 8, 10, 13, 16, 27, 33]}          # model2.py:238-243
# library launches per forward at in_dim 5: seg_input, the extractor's 16, mask_volume, the estimator's 25 (motion_input, ten hourglass
# convs, two resizes, seven encoder convs, the broadcast, fuser, mask, deform, the occlusion conv), the generator's 18 (warp + 17 convs),
# the predictor's 3
LAUNCHES = 1 + EXTRACTOR_LAUNCHES + 1 + 25 + 18 + 3


def seg_input(img, segmap, c0=SEG_CHANNELS[0], c1=SEG_CHANNELS[1], size=None, out=None):
    """r3d_torso_seg_input: cat(img [N, Ci, OH, OW], F.interpolate(segmap[:, [c0, c1]], (OH, OW), mode='bilinear')) [N, Ci + 2, OH, OW];
    img None: the resized pair alone at `size`."""
    seg = _check_f32(segmap, "segmap", 4)
    N, Cs, Hs, Ws = seg.shape
    if img is None:
        Ci, (OH, OW) = 0, size
    else:
        img = _check_f32(img, "img", 4)
        Ci, OH, OW = img.shape[1:]
        if img.shape[0] != N:
            raise ValueError("seg_input: img %s and segmap %s differ in N" % (tuple(img.shape), tuple(seg.shape)))
    if out is None:
        out = torch.empty(N, Ci + 2, OH, OW, device=seg.device, dtype=torch.float32)
    _lib.call("r3d_torso_seg_input", img, N, Ci, seg, Cs, Hs, Ws, c0, c1, out, OH, OW)
    return out


def mask_volume(feats_cl, segmap, c0=SEG_CHANNELS[0], c1=SEG_CHANNELS[1], ksize=7, mul_mask=True, masked_cl=None, motion_cl=None):
    """r3d_torso_mask_volume on feats_cl [N, D, H, W, C]: (masked_cl [N, D, H, W, C], motion_cl [N, D, H, W, C + 2]).  masked_cl may be
    feats_cl (in place)."""
    feats, seg = _check_f32(feats_cl, "feats_cl", 5), _check_f32(segmap, "segmap", 4)
    N, D, H, W, C = feats.shape
    if seg.shape[0] != N:
        raise ValueError("mask_volume: feats_cl %s and segmap %s differ in N" % (tuple(feats.shape), tuple(seg.shape)))
    e = lambda c: torch.empty(N, D, H, W, c, device=feats.device, dtype=torch.float32)
    masked_cl = e(C) if masked_cl is None else masked_cl
    motion_cl = e(C + 2) if motion_cl is None else motion_cl
    _lib.call("r3d_torso_mask_volume", feats, N, D, H, W, C, seg, seg.shape[1], seg.shape[2], seg.shape[3], c0, c1, int(ksize), int(bool(mul_mask)),
              masked_cl, motion_cl)
    return masked_cl, motion_cl


def masked_l1_reg_loss(img_pred, mask, unmasked_weight):
    """model2.py:289-298 (mode 'l1'; the reference overrides masked_weight by 1)."""
    weight_mask = mask.float() + (~mask).float() * unmasked_weight
    return (img_pred.abs().sum(dim=1) * weight_mask).mean()


def losses(occlusion, occlusion_2, target_torso_mask=None, unmask_factor=None):
    """model2.py:264-279 on the returned maps, in torch."""
    alphas = occlusion_2.clamp(1e-5, 1 - 1e-5)
    entropy = torch.mean(-alphas * torch.log2(alphas) - (1 - alphas) * torch.log2(1 - alphas))
    if target_torso_mask is None:
        return {"facev2v/occlusion_reg_l1": occlusion.mean(), "facev2v/occlusion_2_reg_l1": occlusion_2.mean(),
                "facev2v/occlusion_2_weights_entropy": entropy}
    outside = (~target_torso_mask).unsqueeze(1).float()
    m1, m2 = F.interpolate(outside, size=occlusion.shape[-2:]), F.interpolate(outside, size=occlusion_2.shape[-2:])
    return {"facev2v/occlusion_reg_l1": masked_l1_reg_loss(occlusion, m1.bool(), unmask_factor),
            "facev2v/occlusion_2_reg_l1": masked_l1_reg_loss(occlusion_2, m2.bool(), unmask_factor),
            "facev2v/occlusion_2_weights_entropy": entropy}


class TorsoForwardState:
    """What `forward` keeps on the torso model between calls: work buffers per (device, stream, shape) and the Jacobian of the identity
    rotations per (device, N).  No result of a call is among them."""

    def __init__(self):
        self.work, self.identity_j = StreamBuffers(self._new_buffers), {}

    @staticmethod
    def _new_buffers(dev, N, in_dim, H, W, D, h, w, C):
        e = lambda *s: torch.empty(*s, device=dev, dtype=torch.float32)
        return {"x": e(N, in_dim, H, W), "masked_cl": e(N, D, h, w, C), "motion_cl": e(N, D, h, w, C + 2)}

    def jacobian(self, dev, N):
        J = self.identity_j.get((dev, N))
        if J is None:
            eye = torch.eye(3, 3, device=dev).unsqueeze(0).repeat([N, 1, 1])
            J = self.identity_j[(dev, N)] = jacobian(eye, eye.clone())          # what the estimator's forward computes from Rs = Rd = I
        return J


def supported(tm):
    """The torso model carries the three HIP modules `forward` drives."""
    from .torso_appearance import AppearanceFeatureExtractor
    from .torso_generator import Generator
    from .torso_motion import MotionFieldEstimator
    return (isinstance(getattr(tm, "appearance_extractor", None), AppearanceFeatureExtractor)
            and isinstance(getattr(tm, "motion_field_estimator", None), MotionFieldEstimator)
            and isinstance(getattr(tm, "deform_based_generator", None), Generator)
            and callable(getattr(tm, "occlusion_2_predictor", None)))


@torch.no_grad()
def forward(self, torso_src_img, segmap, kp_s, kp_d, tgt_head_img, tgt_head_weights, cal_loss=False, target_torso_mask=None):
    """model2.py:222-287, bound on the torso model by patch_model(torso_forward=True).  kp_s, kp_d [N, 68, 3] in [-1, 1].  Returns
    (deformed_torso_img, ret) with ret's kp_src, kp_drv, occlusion, occlusion_2 (the predictor's), deformed_torso_hid and losses."""
    hp = getattr(self, "hparams", None) or {}
    ext, est, gen = self.appearance_extractor, self.motion_field_estimator, self.deform_based_generator
    kp_num = hp.get("torso_kp_num", est.num_keypoints)
    if kp_num not in KP_INDEX:
        raise NotImplementedError("torso forward: torso_kp_num %r is not 4 or 9 (model2.py:238-245)" % (kp_num,))
    img, seg = _check_f32(torso_src_img, "torso_src_img", 4), _check_f32(segmap, "segmap", 4)          # the reference's segmap.float()
    N, _, H, W = img.shape
    if ext.in_dim not in (3, 5) or img.shape[1] != 3 or seg.shape[0] != N or H % 4 or W % 4:
        raise ValueError("torso forward: expected torso_src_img [N, 3, H, W] with H, W multiples of 4, segmap [N, Cs, Hs, Ws] and an "
                         "extractor of in_dim 3 or 5, got %s, %s and in_dim %d" % (tuple(img.shape), tuple(seg.shape), ext.in_dim))
    state = self._r3d_torso_forward
    D, h, w, C = ext.D, H // 4, W // 4, ext.C
    b = state.work.get(img.device, N, ext.in_dim, H, W, D, h, w, C)
    x = seg_input(img, seg, out=b["x"]) if ext.in_dim == 5 else img          # torso_inp_mode rgb_alpha: read off the extractor's width
    feats_cl = ext.forward_cl(x)
    masked_cl, motion_cl = mask_volume(feats_cl, seg, ksize=hp.get("torso_mask_dilate_ksize", 7), mul_mask=hp.get("mul_torso_mask", True),
                                       masked_cl=b["masked_cl"], motion_cl=b["motion_cl"])
    kp_s, kp_d = kp_s[:, KP_INDEX[kp_num], :], kp_d[:, KP_INDEX[kp_num], :]
    deformation, occlusion, occlusion_2 = est.forward_cl(motion_cl, kp_s, kp_d, None, None, tgt_head_img, tgt_head_weights,
                                                         J=state.jacobian(img.device, N))
    ret = {"kp_src": kp_s, "kp_drv": kp_d, "occlusion": occlusion, "occlusion_2": occlusion_2}
    deformed_torso_img, hid = gen.forward_cl(masked_cl, deformation, occlusion, return_hid=True)
    ret["deformed_torso_hid"] = hid
    occlusion_2 = self.occlusion_2_predictor(torch.cat([hid, F.interpolate(occlusion_2, size=(256, 256), mode="bilinear")], dim=1))
    ret["occlusion_2"] = occlusion_2
    ret["losses"] = losses(occlusion, occlusion_2, target_torso_mask,
                           None if target_torso_mask is None else hp["torso_occlusion_reg_unmask_factor"])
    return deformed_torso_img, ret
