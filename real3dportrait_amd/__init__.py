"""MI355X-native tri-plane NeRF volume renderer + super-resolution for Real3D-Portrait's per-frame path.

Operators keep the reference's names and signatures (see each module's docstring for file:line):
    RaySampler, ImportanceRenderer, OSGDecoder          (volumetric_rendering.py)
    SynthesisBlock, SuperresolutionHybrid8XDC           (superresolution.py)
    SynthesisBlockNoUp, Conv2d, ConvStack                (superresolution.py: torso/background fusion convs)
    TriPlaneGenerator (.synthesis contract), patch_model (triplane.py)
    SegFormerSECC2PlaneBackbone                          (segformer.py: the per-frame SECC encoder, mode b0)
    Img2PlaneModel                                       (img2plane.py: the canonical image-to-plane backbone without its DeepLabV3;
                                                         patch_model(cano_backbone=True) installs it)
    DeepLabV3                                            (deeplabv3.py: the backbone's low-resolution encoder, a dilated ResNet + ASPP;
                                                         patch_model(cano_backbone=True, cano_low_reso_encoder=True) installs it)
    Plane2GridModule                                     (plane2grid.py: the Conv3d residual blocks that make tri-grids of the planes;
                                                         patch_model(plane2grid=True) installs it)
    TorsoGenerator, Occlusion2Predictor                  (torso_generator.py: the torso network's warp + decoder, its Generator)
    TorsoMotionFieldEstimator                            (torso_motion.py: the torso network's per-frame MotionFieldEstimator)
    TorsoAppearanceFeatureExtractor                      (torso_appearance.py: the torso network's AppearanceFeatureExtractor)
    torso_model_forward, torso_seg_input, torso_mask_volume (torso_forward.py: the torso model's forward over the three, its two glue kernels)
    MeshRenderer, rasterize, patch_secc_renderer         (mesh_renderer.py: the SECC map's z-buffer rasteriser, without pytorch3d)
    blink_eye_for_secc, blink_frames, apply_periodic_blink, blink_schedule, patch_blink (edit_secc.py: the driving maps' blink edit)
    compute_face_vertex, reconstruct_lm2d, patch_face_model, patch_face3d_helper (face_model.py: the morphable model's vertices and landmarks)
    get_driving_motion, patch_driving_motion             (driving_motion.py: face model -> rasteriser -> blink -> landmarks on the device)
    clip_camera, camera_pose_intrinsic, smooth_camera_sequence, smooth_features_xd, clip_keypoints, patch_infer_utils
                                                         (clip_conditions.py: the clip's camera trajectory and smoothed key points)
    depth_range, compose_debug_frames, clip_frames, secc2video_frames, write_video, patch_secc2video
                                                         (video_frames.py: the clip's output frames, out_mode 'final' and 'concat_debug')
    nearest_seed, head_image, inpaint_torso_job, extract_background, source_to_planes, patch_segment_imgs
                                                         (source_conditions.py: the source image's head, torso and background conditions;
                                                         the name source_conditions is the module, its function source_conditions.source_conditions)
    PitchContourVAEModel, VAEModel, patch_audio2secc     (audio2motion.py: the audio-to-motion VAE behind forward_audio2secc)
    HubertFeatureModel, hubert_features, chunk_plan, get_hubert, patch_hubert (hubert.py: the HuBERT audio features behind get_hubert)
    landmark_weights, fit_landmarks, fit_3dmm_for_landmarks, patch_fit_3dmm (fit_3dmm.py: the landmark-driven 3DMM fit, 400 Adam steps)
    render_clip_sharded                                  (frames.py: frame sharding + RCCL gather)
All compute goes through libr3d_hip.so (include/r3d_hip.h, include/r3d_hip_img2plane.h, include/r3d_hip_hubert.h,
include/r3d_hip_deeplab.h, include/r3d_hip_plane2grid.h); there is no eager/CPU fallback.
"""
__version__ = "0.1.0"


def __getattr__(name):      # lazy: importing the package (e.g. for synth) must not require torch+GPU
    if name in ("RaySampler", "ImportanceRenderer", "OSGDecoder"):
        from . import volumetric_rendering as m
        return getattr(m, name)
    if name in ("SynthesisBlock", "SuperresolutionHybrid8XDC", "SynthesisBlockNoUp", "Conv2d", "ConvStack"):
        from . import superresolution as m
        return getattr(m, name)
    if name in ("TriPlaneGenerator", "patch_model"):
        from . import triplane as m
        return getattr(m, name)
    if name == "SegFormerSECC2PlaneBackbone":
        from . import segformer as m
        return getattr(m, name)
    if name == "Img2PlaneModel":
        from . import img2plane as m
        return getattr(m, name)
    if name == "DeepLabV3":
        from . import deeplabv3 as m
        return m.DeepLabV3
    if name == "Plane2GridModule":
        from . import plane2grid as m
        return m.Plane2GridModule
    if name in ("TorsoGenerator", "Occlusion2Predictor"):
        from . import torso_generator as m
        return getattr(m, "Generator" if name == "TorsoGenerator" else name)
    if name == "TorsoMotionFieldEstimator":
        from . import torso_motion as m
        return m.MotionFieldEstimator
    if name == "TorsoAppearanceFeatureExtractor":
        from . import torso_appearance as m
        return m.AppearanceFeatureExtractor
    if name in ("torso_model_forward", "torso_seg_input", "torso_mask_volume"):
        import importlib
        m = importlib.import_module(".torso_forward", __name__)          # the submodule's name is not an attribute this function serves
        return getattr(m, {"torso_model_forward": "forward", "torso_seg_input": "seg_input", "torso_mask_volume": "mask_volume"}[name])
    if name in ("MeshRenderer", "rasterize", "patch_secc_renderer"):
        import importlib
        return getattr(importlib.import_module(".mesh_renderer", __name__), name)
    if name in ("blink_eye_for_secc", "blink_frames", "blink_schedule", "apply_periodic_blink", "patch_blink"):
        import importlib
        return getattr(importlib.import_module(".edit_secc", __name__), name)
    if name in ("compute_face_vertex", "reconstruct_lm2d", "patch_face_model", "patch_face3d_helper"):
        import importlib
        return getattr(importlib.import_module(".face_model", __name__), name)
    if name in ("get_driving_motion", "patch_driving_motion"):
        import importlib
        return getattr(importlib.import_module(".driving_motion", __name__), name)
    if name in ("camera_pose_intrinsic", "smooth_camera_sequence", "clip_camera", "smooth_features_xd", "clip_keypoints", "patch_infer_utils"):
        import importlib
        return getattr(importlib.import_module(".clip_conditions", __name__), name)
    if name in ("depth_range", "compose_debug_frames", "clip_frames", "secc2video_frames", "write_video", "patch_secc2video"):
        import importlib
        return getattr(importlib.import_module(".video_frames", __name__), name)
    if name in ("nearest_seed", "head_image", "inpaint_torso_job", "extract_background", "source_to_planes", "patch_segment_imgs"):
        import importlib
        return getattr(importlib.import_module(".source_conditions", __name__), name)
    if name in ("PitchContourVAEModel", "VAEModel", "patch_audio2secc"):
        import importlib
        return getattr(importlib.import_module(".audio2motion", __name__), name)
    if name in ("HubertFeatureModel", "hubert_features", "chunk_plan", "get_hubert", "patch_hubert"):
        import importlib
        return getattr(importlib.import_module(".hubert", __name__), name)
    if name in ("landmark_weights", "fit_landmarks", "fit_3dmm_for_landmarks", "patch_fit_3dmm"):
        import importlib
        return getattr(importlib.import_module(".fit_3dmm", __name__), name)
    if name in ("render_clip_sharded", "shard_frames"):
        from . import frames as m
        return getattr(m, name)
    raise AttributeError(name)
