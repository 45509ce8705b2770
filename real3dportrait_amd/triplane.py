"""Generator shell with the reference's `TriPlaneGenerator.synthesis()` contract, HIP hot path inside.

Mirrors modules/eg3ds/models/triplane.py:23-163 for everything downstream of the tri-plane tensor:
`synthesis(ws, camera, cond=None, update_emas=False, cache_backbone=False, use_cached_backbone=False,
**synthesis_kwargs)` returns {'image','image_raw','image_depth','image_feature','plane'} with the same shapes.
The tri-plane producer (StyleGAN2 backbone / img2plane / secc2plane) is a cold PyTorch encoder and stays
outside: pass it as `backbone` (any module with `.synthesis(ws, **kw) -> [N,96,256,256]`) or inject planes
through `_last_planes` + use_cached_backbone=True exactly like the reference's inference loop does
(inference/real3d_infer.py:486-489).

`patch_model(model)` swaps ray_sampler / renderer / superresolution of an already-constructed reference
model (TriPlaneGenerator, OSAvatar_Img2plane, OSAvatarSECC_Img2plane[_Torso]) for the HIP operators,
keeping its parameters (strict state_dict copy).
"""
import copy

import torch
import torch.nn as nn

from .superresolution import SuperresolutionHybrid8XDC, SynthesisBlock, const_bound
from .volumetric_rendering import ImportanceRenderer, OSGDecoder, RaySampler

DEFAULT_HPARAMS = {           # egs/egs_bases/eg3d/base.yaml:20-44 (+ 'auto' limits as every os_avatar config sets)
    "final_resolution": 512, "neural_rendering_resolution": 128, "num_samples_coarse": 48, "num_samples_fine": 48,
    "ray_near": "auto", "ray_far": "auto", "box_warp": 1.0, "w_dim": 512, "base_channel": 32768, "max_channel": 512,
    "ones_ws_for_sr": True, "mask_invalid_rays": False, "triplane_feature_type": "triplane",
}


class TriPlaneGenerator(nn.Module):
    def __init__(self, hp=None, backbone=None):
        super().__init__()
        self.hparams = copy.copy(DEFAULT_HPARAMS)
        if hp is not None:
            self.hparams.update(hp)
        hparams = self.hparams
        self.camera_dim = 25
        self.w_dim = hparams["w_dim"]
        self.img_resolution = hparams["final_resolution"]
        self.img_channels = 3
        self.renderer = ImportanceRenderer(hp=hparams)
        self.renderer.triplane_feature_type = "triplane"
        self.ray_sampler = RaySampler()
        self.neural_rendering_resolution = hparams["neural_rendering_resolution"]
        self.backbone = backbone
        self.decoder = OSGDecoder(32, {"decoder_lr_mul": 1, "decoder_output_dim": 32})
        self.rendering_kwargs = {
            "image_resolution": hparams["final_resolution"], "disparity_space_sampling": False,
            "clamp_mode": "softplus", "c_scale": 1.0, "superresolution_noise_mode": "none", "sr_antialias": True,
            "depth_resolution": hparams["num_samples_coarse"],
            "depth_resolution_importance": hparams["num_samples_fine"],
            "ray_start": hparams["ray_near"], "ray_end": hparams["ray_far"], "box_warp": hparams["box_warp"],
            "avg_camera_radius": 2.7, "avg_camera_pivot": [0, 0, 0.2], "white_back": False,
        }
        self.superresolution = SuperresolutionHybrid8XDC(
            channels=32, img_resolution=self.img_resolution, sr_num_fp16_res=0, sr_antialias=True,
            channel_base=hparams["base_channel"], channel_max=hparams["max_channel"],
            fused_modconv_default="inference_only")
        self._last_planes = None
        self._ones_ws = None

    # -- the reference's public surface (modules/eg3ds/models/triplane.py:73-163) -------------------------------------
    def mapping(self, z, camera, cond=None, truncation_psi=0.7, truncation_cutoff=None, update_emas=False):
        """triplane.py:73-88: the mapping network lives in the (cold, PyTorch) tri-plane producer."""
        if self.backbone is None or not hasattr(self.backbone, "mapping"):
            raise RuntimeError("mapping() needs a backbone with a mapping network (the StyleGAN2 producer is a cold encoder, out of scope)")
        ws = self.backbone.mapping(z, camera * self.rendering_kwargs.get("c_scale", 0), truncation_psi=truncation_psi,
                                   truncation_cutoff=truncation_cutoff, update_emas=update_emas)
        if self.hparams.get("gen_cond_mode", "none") == "mapping":        # triplane.py:85-87
            d_ws = self.backbone.cond_mapping(cond, None, truncation_psi=truncation_psi, truncation_cutoff=truncation_cutoff,
                                              update_emas=update_emas)
            ws = ws * 0.5 + d_ws * 0.5
        return ws

    def _planes(self, ws, update_emas, cache_backbone, use_cached_backbone, synthesis_kwargs):
        if use_cached_backbone and self._last_planes is not None:
            planes = self._last_planes
        elif self.backbone is None:
            raise RuntimeError("no tri-plane producer: pass backbone=... or set _last_planes and use_cached_backbone=True")
        else:
            planes = self.backbone.synthesis(ws, update_emas=update_emas, **synthesis_kwargs)
        if cache_backbone:
            self._last_planes = planes
        return planes.view(len(planes), 3, -1, planes.shape[-2], planes.shape[-1])

    def _ray_images(self, planes, camera, sr_ws=None):
        """Rays -> fused HIP renderer -> the 'raw' neural-rendered images [N,C,R,R] (triplane.py:96-127 / secc_img2plane.py:99-130).
        sr_ws: the ws the SR will be called with next; when the SR is the HIP one and takes R^2 inputs as they come, the ray kernel
        also writes its first operand (images["feature_split"], ImportanceRenderer.forward `_split_for`)."""
        R = self.neural_rendering_resolution
        c2w, K = camera[:, :16].view(-1, 4, 4), camera[:, 16:25].view(-1, 3, 3)
        split = None
        if type(self.ray_sampler) is RaySampler and type(self.renderer) is ImportanceRenderer:
            # both operators are the HIP ones: the rays are generated inside the render launches (same pixels, triplane.py:96-99 + :113)
            sr = self.superresolution
            spec = None
            if (sr_ws is not None and isinstance(sr, SuperresolutionHybrid8XDC) and R == sr.input_resolution
                    and not self.hparams.get("mask_invalid_rays", False)):          # (the mask edits the fp32 image afterwards)
                spec = sr.split_input_spec(sr_ws, c2w.shape[0], c2w.device)
            feat, depth, wsum, valid = self.renderer.forward_camera(planes, self.decoder, c2w, K, R, self.rendering_kwargs, _split_for=spec)
            split = getattr(feat, "_r3d_split", None)
        else:
            origins, directions = self.ray_sampler(c2w, K, R)
            feat, depth, wsum, valid = self.renderer(planes, self.decoder, origins, directions, self.rendering_kwargs)   # [N, R*R, C]
        N = feat.shape[0]
        to_img = lambda t: t.transpose(1, 2).reshape(N, t.shape[-1], R, R)
        images = {"feature": to_img(feat).contiguous(), "depth": to_img(depth), "weights": to_img(wsum).contiguous(), "feature_split": split}
        if self.hparams.get("mask_invalid_rays", False):
            # feature <- -1 and depth <- min valid depth on rays that miss the box (triplane.py:123-126), without the
            # reference's host sync (.item()) and boolean indexing
            keep = valid.reshape(N, 1, R, R)
            d = images["depth"]
            dmin = torch.where(keep, d, torch.full_like(d, float("inf"))).amin()
            images["feature"] = torch.where(keep, images["feature"], torch.full_like(images["feature"], -1.0))
            images["depth"] = torch.where(keep, d, dmin)
        return images

    def _ws_for_sr(self, ws):
        if not self.hparams["ones_ws_for_sr"]:
            return ws
        c = self._ones_ws
        if c is None or c.shape != ws.shape or c.device != ws.device:
            c = self._ones_ws = torch.ones_like(ws)       # one persistent tensor: the SR blocks cache their style vectors on it
        return c

    def synthesis(self, ws, camera, cond=None, update_emas=False, cache_backbone=False, use_cached_backbone=False,
                  **synthesis_kwargs):
        """triplane.py:90-138.  Returns the reference's keys plus 'weights_img' (the name the Real3D shells use,
        secc_img2plane.py:132)."""
        planes = self._planes(ws, update_emas, cache_backbone, use_cached_backbone, synthesis_kwargs)
        sr_ws = self._ws_for_sr(ws)
        sr_kwargs = {k: v for k, v in synthesis_kwargs.items() if k != "noise_mode"}
        im = self._ray_images(planes, camera, sr_ws=None if sr_kwargs else sr_ws)
        feature = im["feature"]
        # |feature| <= 1.002 by construction (sigmoid * 1.002 - 0.001 composited with weights summing to <= 1, then * 2 - 1):
        # the SR's fp16 range fold uses this bound instead of measuring it
        feature._r3d_bound, feature._r3d_depth = const_bound(1.01, feature.shape[0], feature.device), 0
        x = im["feature_split"] if im.get("feature_split") is not None else feature
        sr_image = self.superresolution(feature[:, :3], x, sr_ws,
                                        noise_mode=self.rendering_kwargs["superresolution_noise_mode"], **sr_kwargs)
        return {"image": sr_image.clamp(-1, 1), "image_raw": feature[:, :3].clamp(-1, 1), "image_depth": im["depth"],
                "image_feature": feature[:, 3:], "plane": planes, "weights_img": im["weights"]}

    def sample(self, coordinates, directions, z, camera, cond=None, truncation_psi=1, truncation_cutoff=None, update_emas=False,
               **synthesis_kwargs):
        """triplane.py:140-148."""
        ws = self.mapping(z, camera, cond=cond, truncation_psi=truncation_psi, truncation_cutoff=truncation_cutoff, update_emas=update_emas)
        return self.sample_mixed(coordinates, directions, ws, update_emas=update_emas, **synthesis_kwargs)

    def sample_mixed(self, coordinates, directions, ws, truncation_psi=1, truncation_cutoff=None, update_emas=False,
                     **synthesis_kwargs):
        """triplane.py:150-156."""
        planes = self.backbone.synthesis(ws, update_emas=update_emas, **synthesis_kwargs)
        planes = planes.view(len(planes), 3, -1, planes.shape[-2], planes.shape[-1])
        return self.renderer.run_model(planes, self.decoder, coordinates, directions, self.rendering_kwargs)

    def forward(self, z, camera, cond=None, truncation_psi=1, truncation_cutoff=None, neural_rendering_resolution=None,
                update_emas=False, cache_backbone=False, use_cached_backbone=False, **synthesis_kwargs):
        """triplane.py:158-163: mapping -> synthesis."""
        ws = self.mapping(z, camera, cond=cond, truncation_psi=truncation_psi, truncation_cutoff=truncation_cutoff, update_emas=update_emas)
        return self.synthesis(ws, camera, cond=cond, update_emas=update_emas, cache_backbone=cache_backbone,
                              use_cached_backbone=use_cached_backbone, **synthesis_kwargs)


def _reference_hparams(model):
    """The reference keeps its configuration in one global dict (utils/commons/hparams.py) that its modules read at call time;
    some shells also keep a copy as `self.hparams`."""
    import sys
    hp = {}
    mod = sys.modules.get("utils.commons.hparams")
    if mod is not None and isinstance(getattr(mod, "hparams", None), dict):
        hp.update(mod.hparams)
    if isinstance(getattr(model, "hparams", None), dict):
        hp.update(model.hparams)
    return hp


def patch_model(model, fuse_warp_sr=True, precision=None, secc_encoder=False, torso_generator=False, torso_motion=False, torso_precision=None,
                torso_appearance=False, torso_forward=False, cano_backbone=False, cano_low_reso_encoder=False, plane2grid=False):
    """Swap the hot-path operators of a constructed reference model for the HIP ones (in place).  INFERENCE ONLY: the HIP modules
    detach their inputs and build no autograd graph (the reference runs this path under torch.no_grad(), real3d_infer.py:435,479).
    precision: SR precision of the installed blocks (None = the library default 'f16mx': inside the 2e-4 of SURVEY 8(d) on every golden and heavy-tail sweep,
    what bench.py measures; 'f16x3' = the fp32-class tier, 1.3e-6; superresolution.py "Precision policy").

    * model.ray_sampler  -> RaySampler            (created at img2plane_baseline.py:106 / triplane.py:38)
    * model.renderer     -> ImportanceRenderer    (img2plane_baseline.py:104-105 / triplane.py:36-37)
    * model.superresolution (vanilla SuperresolutionHybrid8XDC) -> HIP SuperresolutionHybrid8XDC, or, for the
      torso model whose superresolution is SuperresolutionHybrid8XDC_Warp (secc_img2plane_torso.py:10-11),
      its .block0 / .block1 (called at sr_with_ref.py:83,124 as block(x, img, ws, **kw) -> (x, img)), its torso / background
      fusion stacks (nn.Sequential -> ConvStack, :24-63) and head_torso_block (-> SynthesisBlockNoUp); with fuse mode 'v2' and
      fuse_warp_sr=True its forward is replaced by the fused HIP evaluation (real3dportrait_amd/sr_with_ref.py).
      With hparams weight_fuse=False the reference calls block1(x, None, ws) (sr_with_ref.py:161), which the HIP block does not
      cover: block1 is then left untouched.
    * <backbone>.to_plane_cnn (segformer.py:691-700) -> ConvStack.
    * secc_encoder=True (opt-in): model.secc_img2plane_backbone, when it is the reference's SegFormerSECC2PlaneBackbone in mode b0
      (segformer.py:672-731), -> the HIP SegFormerSECC2PlaneBackbone (segformer.py of this package: prenet, MiT-b0 and the head in
      exact fp32, to_plane_cnn as a ConvStack).  Other backbones are left as they are.
    * torso_generator=True (opt-in): model.superresolution.torso_model.deform_based_generator, when it is the reference's Generator at
      standard / small scale (facev2v_warp/network2.py:248-301), -> the HIP Generator, and torso_model.occlusion_2_predictor
      (model2.py:212-219) -> the HIP Occlusion2Predictor (torso_generator.py of this package: the warp and every conv in exact fp32).
      torso_model.forward and infer_forward_stage2 reach them unchanged.  Other generators are left as they are.
    * torso_motion=True (opt-in): model.superresolution.torso_model.motion_field_estimator, when it is the reference's v2
      MotionFieldEstimator at standard scale (facev2v_warp/network2.py:162-244, with the target-head branch), -> the HIP
      MotionFieldEstimator (torso_motion.py of this package: the Conv3d hourglass, the fuser, the mask and the occlusion maps in exact
      fp32).  torso_model.forward reaches it unchanged (model2.py:250).  The v1 estimator of network.py (no target-head branch) and
      anything else are left as they are.
    * torso_appearance=True (opt-in): model.superresolution.torso_model.appearance_extractor, when it is the reference's
      AppearanceFeatureExtractor (facev2v_warp/network2.py:16-45), -> the HIP AppearanceFeatureExtractor (torso_appearance.py of this
      package: every conv in exact fp32, 16 launches per call).  torso_model.forward reaches it unchanged, on every frame
      (model2.py:230); nothing is cached across calls.  Anything else is left as it is.
    * torso_precision: the tier of the convolutions of the modules the three torso switches install (torso_precision.py): None = 'f32',
      every product on the fp32 matrix instruction (the exact tier, the default and the recommendation); 'bf16x3' = each operand split into
      three bf16 pieces and six piece products summed in fp32, fp32-class, no range state.  Given without torso_generator, torso_motion or
      torso_appearance it is a ValueError, as is an unknown name.
    * torso_forward=True (opt-in; needs torso_appearance=True, torso_motion=True and torso_generator=True, anything else is a
      ValueError): model.superresolution.torso_model.forward (facev2v_warp/model2.py:222-287) -> torso_forward.py's forward of this
      package, with the reference's signature and `ret`: the glue of model2.py:226-236 in two HIP launches (r3d_torso_seg_input,
      r3d_torso_mask_volume) and the appearance volume channel-last from the extractor to the estimator and the generator, 64 library
      launches per call.  rgb_alpha or not is read from the installed extractor's input width; torso_kp_num, torso_mask_dilate_ksize and
      mul_torso_mask from torso_model.hparams.  Still torch: the key-point index select, cat([tgt_head_img, tgt_head_weights]) inside the
      estimator, the interpolate + cat in front of occlusion_2_predictor, and the losses.  Every call computes everything; nothing is
      cached across calls.  If one of the three swaps was refused for this model, forward is left as it is; infer_forward_stage1 / 2
      always are.  The reference's forward stays reachable as torso_model._r3d_reference_forward.
    * cano_backbone=True (opt-in): model.cano_img2plane_backbone (OSAvatarSECC_Img2plane, secc_img2plane.py:29,50-62), or
      model.img2plane_backbone on OSAvatar_Img2plane, when -- and only when -- it is the reference's Img2PlaneModel
      (modules/img2plane/img2plane_model.py:12-82), -> the HIP Img2PlaneModel (img2plane.py of this package: HighResoEncoder,
      LowResolutionViT and TriplanePredictorViT in exact fp32).  Its low_reso_encoder (DeepLabV3) is the reference's own object and stays
      torch, as does the input assembly, unless cano_low_reso_encoder is given.  The replaced module stays reachable as
      model._r3d_reference_cano_backbone.  Anything else is left as it is.
    * cano_low_reso_encoder=True (opt-in; needs cano_backbone=True, anything else is a ValueError): the installed backbone's
      low_reso_encoder, when it is the reference's DeepLabV3 over a BasicBlock ResNet at output stride 8 (deeplabv3.py's from_reference
      reads stride, dilation and padding from each of its Conv2d objects), -> the HIP DeepLabV3, and the backbone's forward then assembles
      its input with r3d_dl_assemble_input and runs channel-last throughout: no torch.nn.Conv2d runs inside the backbone.  The alpha
      threshold and the camera Linear stay torch.  The old encoder stays reachable as <backbone>._r3d_reference_low_reso_encoder.  Any
      other encoder is left as it is.
    * plane2grid=True (opt-in; independent of cano_backbone): model.plane2grid_module (img2plane_baseline.py:96-97, the trigrid_v2 models),
      when it is the reference's Plane2GridModule at the renderer's width (in_out_dim 96, 32 channels per plane), -> the HIP
      Plane2GridModule (plane2grid.py of this package: GroupNorm statistics and the replicate-padded Conv3d in exact fp32).  cal_plane /
      cal_cano_plane reach it unchanged.  The old module stays reachable as model._r3d_reference_plane2grid_module.  Anything else, and a
      model without the attribute, is left as it is.
    Parameters are copied with strict key matching; the decoder module is left untouched (the renderer reads
    decoder.net[0|2].{weight,bias} directly)."""
    import types
    from .torso_precision import F32, check_precision
    if torso_precision is not None and not (torso_generator or torso_motion or torso_appearance):
        raise ValueError("patch_model: torso_precision=%r needs torso_generator=True, torso_motion=True or torso_appearance=True" % (torso_precision,))
    torso_precision = check_precision(F32 if torso_precision is None else torso_precision, "patch_model: torso_precision")
    if torso_forward and not (torso_appearance and torso_motion and torso_generator):
        raise ValueError("patch_model: torso_forward=True needs torso_appearance=True, torso_motion=True and torso_generator=True (got %r, %r, %r): "
                         "it drives the three HIP modules" % (torso_appearance, torso_motion, torso_generator))
    if cano_low_reso_encoder and not cano_backbone:
        raise ValueError("patch_model: cano_low_reso_encoder=True needs cano_backbone=True: it swaps the encoder of the backbone that switch installs")
    dev = next(model.parameters()).device
    hp = _reference_hparams(model)
    old_r = model.renderer
    new_r = ImportanceRenderer(hp=getattr(old_r, "hparams", None))
    new_r.triplane_feature_type = getattr(old_r, "triplane_feature_type", "triplane")
    model.renderer = new_r
    model.ray_sampler = RaySampler()
    sr = model.superresolution
    if type(sr).__name__ == "SuperresolutionHybrid8XDC":
        new_sr = SuperresolutionHybrid8XDC(channels=sr.block0.in_channels, img_resolution=512, sr_num_fp16_res=0,
                                           sr_antialias=sr.sr_antialias).to(dev)
        new_sr.load_state_dict(sr.state_dict(), strict=True)
        model.superresolution = new_sr
    else:
        weight_fuse = bool(hp.get("weight_fuse", True))
        for name in ("block0", "block1"):
            old = getattr(sr, name, None)
            if old is None or type(old).__name__ != "SynthesisBlock" or (name == "block1" and not weight_fuse):
                continue
            new = SynthesisBlock(old.in_channels, old.conv1.out_channels, w_dim=old.w_dim, resolution=old.resolution,
                                 img_channels=old.img_channels, is_last=old.is_last, use_fp16=False,
                                 conv_clamp=old.conv1.conv_clamp).to(dev)
            new.load_state_dict(old.state_dict(), strict=True)
            setattr(sr, name, new)
        _patch_fusion_stacks(sr, dev)
        if (fuse_warp_sr and weight_fuse and hp.get("htbsr_head_weight_fuse_mode") == "v2" and hasattr(sr, "torso_model")
                and type(getattr(sr, "head_torso_block", None)).__name__ == "SynthesisBlockNoUp"
                and type(sr.head_torso_block).__module__.startswith("real3dportrait_amd")):
            from . import sr_with_ref
            # snapshot of the keys the fused forward reads -- only those that are SET (absent keys keep the reference's defaults, e.g.
            # torso_model_version 'v1', sr_with_ref.py:84); the reference reads its global hparams at call time, so patch_model must
            # run after set_hparams()
            sr._r3d_state = sr_with_ref.WarpSRState(
                {k: hp[k] for k in ("weight_fuse", "htbsr_head_weight_fuse_mode", "htbsr_head_threshold", "torso_model_version") if k in hp})
            sr._r3d_reference_forward = sr.forward           # the exact-f32 precision runs the reference forward over the patched sub-modules
            sr.forward = types.MethodType(sr_with_ref.forward_v2, sr)
            sr.split_input_spec = types.MethodType(sr_with_ref.warp_split_input_spec, sr)
    if secc_encoder:
        bb = getattr(model, "secc_img2plane_backbone", None)
        if (type(bb).__name__ == "SegFormerSECC2PlaneBackbone" and not type(bb).__module__.startswith("real3dportrait_amd")
                and getattr(bb, "mode", None) == "b0"):
            from .segformer import SegFormerSECC2PlaneBackbone as HipSECC
            model.secc_img2plane_backbone = HipSECC.from_reference(bb)
    if torso_generator:
        from . import torso_generator as tg
        tm = getattr(model.superresolution, "torso_model", None)
        if tm is not None and tg.is_reference_generator(getattr(tm, "deform_based_generator", None)):
            tm.deform_based_generator = tg.Generator.from_reference(tm.deform_based_generator, torso_precision)
            if tg.is_reference_predictor(getattr(tm, "occlusion_2_predictor", None)):
                tm.occlusion_2_predictor = tg.Occlusion2Predictor.from_reference(tm.occlusion_2_predictor, torso_precision)
    if torso_motion:
        from . import torso_motion as tmo
        tm = getattr(model.superresolution, "torso_model", None)
        if tm is not None and tmo.is_reference_motion_estimator(getattr(tm, "motion_field_estimator", None)):
            tm.motion_field_estimator = tmo.MotionFieldEstimator.from_reference(tm.motion_field_estimator, torso_precision)
    if torso_appearance:
        from . import torso_appearance as tap
        tm = getattr(model.superresolution, "torso_model", None)
        if tm is not None and tap.is_reference_appearance_extractor(getattr(tm, "appearance_extractor", None)):
            tm.appearance_extractor = tap.AppearanceFeatureExtractor.from_reference(tm.appearance_extractor, torso_precision)
    if torso_forward:
        from . import torso_forward as tf
        tm = getattr(model.superresolution, "torso_model", None)
        if tm is not None and tf.supported(tm):
            tm._r3d_torso_forward = tf.TorsoForwardState()
            tm._r3d_reference_forward = tm.forward
            tm.forward = types.MethodType(tf.forward, tm)
    if cano_backbone:
        from . import img2plane as i2p
        for name in ("cano_img2plane_backbone", "img2plane_backbone"):
            bb = getattr(model, name, None)
            if i2p.is_reference_img2plane(bb):
                object.__setattr__(model, "_r3d_reference_cano_backbone", bb)        # reachable, not registered as a second sub-module
                new = i2p.Img2PlaneModel.from_reference(bb)
                setattr(model, name, new)
                if cano_low_reso_encoder:
                    from . import deeplabv3 as dl
                    old = new.low_reso_encoder
                    enc = dl.DeepLabV3.from_reference(old) if dl.is_reference_deeplabv3(old) else None
                    if enc is not None and enc.in_channels == new.in_channels and enc.out_channels == 256:
                        object.__setattr__(new, "_r3d_reference_low_reso_encoder", old)        # reachable, not a second sub-module
                        new.low_reso_encoder = enc
                break
    if plane2grid:
        from . import plane2grid as p2g
        old = getattr(model, "plane2grid_module", None)
        new = p2g.Plane2GridModule.from_reference(old) if p2g.is_reference_plane2grid(old) else None
        if new is not None:
            object.__setattr__(model, "_r3d_reference_plane2grid_module", old)        # reachable, not registered as a second sub-module
            model.plane2grid_module = new
    for owner in (getattr(model, "secc_img2plane_backbone", None), getattr(model, "img2plane_backbone", None)):
        _patch_sequential(owner, "to_plane_cnn", dev)       # per-frame plane producer tail (segformer.py:691-700)
    from .superresolution import set_sr_precision
    set_sr_precision(model.superresolution, precision)
    return model


def _patch_sequential(owner, name, dev):
    """owner.<name>: nn.Sequential of Conv2d / LeakyReLU / UpsamplingBilinear2d(2) -> ConvStack (same state_dict keys, NCHW in
    and out, so the surrounding reference code is unchanged).  Stacks the HIP conv does not cover are left alone."""
    from .superresolution import ConvStack
    seq = getattr(owner, name, None) if owner is not None else None
    if seq is None or type(seq).__name__ != "Sequential":
        return False
    try:
        setattr(owner, name, ConvStack.from_torch(seq).to(dev))
    except NotImplementedError:
        return False
    return True


def _patch_fusion_stacks(sr, dev):
    """SuperresolutionHybrid8XDC_Warp (sr_with_ref.py:24-63): the torso / background fusion stacks and head_torso_block."""
    from .superresolution import SynthesisBlockNoUp
    for name in ("torso_encoder", "bg_encoder", "fuse_head_torso_convs", "fuse_fg_bg_convs"):
        _patch_sequential(sr, name, dev)
    old = getattr(sr, "head_torso_block", None)
    if old is not None and type(old).__name__ == "SynthesisBlockNoUp":
        new = SynthesisBlockNoUp(old.in_channels, old.conv1.out_channels, w_dim=old.w_dim, resolution=old.resolution,
                                 img_channels=old.img_channels, is_last=old.is_last, use_fp16=False,
                                 conv_clamp=old.conv1.conv_clamp).to(dev)
        new.load_state_dict(old.state_dict(), strict=True)
        sr.head_torso_block = new
