"""Regenerate the img2plane_* golden vectors: the reference's Img2PlaneModel (modules/img2plane/img2plane_model.py:12-82) on CPU in fp32,
its own __init__ and forward, with the synthetic weights of real3dportrait_amd.synth.synth_img2plane and the inputs of
tests/img2plane_common.py.

Run in the build container only (needs the reference tree, R3D_REFERENCE):
    python tests/golden/make_golden_img2plane.py
Inputs and weights are regenerated from the seeds of img2plane_common.CASES, so the fixtures hold only outputs.

The reference imports timm (stand-ins as in make_golden_secc.py: DropPath, to_2tuple, trunc_normal_) and its DeepLabV3 package, whose
imports (torchvision, pretrainedmodels) are not installed and whose constructor fetches ImageNet weights.  That package is never imported:
a stand-in module `modules.img2plane.deeplabv3` is put into sys.modules before modules.img2plane.img2plane_model is, and its
DeepLabV3(in_channels=...) returns img2plane_common.StandInEncoder.

Stored per case: the planes, four sub-sampled taps (img2plane_common.TAP_SLICES), and `attention` [n, 2]: per attention its number of
keys L and the median over query rows of the largest softmax probability, which the maker requires to lie in (2 / L, 0.9) -- neither
uniform nor one-hot -- measured by the fp64 restatement (tests/img2plane_ref64.py), which the maker also requires to meet the reference
within 2e-4 of max|ref|.  On every reference model it constructs, the maker also runs the package's Img2PlaneModel.from_reference
(check_from_reference): the attributes that method reads are the real class's."""
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("R3D_REFERENCE", "/root/reference")
sys.path.insert(0, REF)
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, HERE)

import img2plane_common as common  # noqa: E402
import img2plane_ref64 as R64  # noqa: E402
from real3dportrait_amd import synth  # noqa: E402


def _install_stand_ins():
    import ref_stubs
    ref_stubs.install()
    layers = types.ModuleType("timm.models.layers")

    class DropPath(nn.Module):
        def __init__(self, p=0.0):
            super().__init__()
            self.drop_prob = p

        def forward(self, x):
            return x

    layers.DropPath = DropPath
    layers.to_2tuple = lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v, v)
    layers.trunc_normal_ = lambda t, std=1.0, **k: nn.init.normal_(t, std=std)
    sys.modules["timm.models.layers"] = layers
    deeplab = types.ModuleType("modules.img2plane.deeplabv3")
    deeplab.DeepLabV3 = lambda in_channels=3, **k: common.StandInEncoder(in_channels)
    sys.modules["modules.img2plane.deeplabv3"] = deeplab


def reference_model(mode, scale, sd):
    _install_stand_ins()
    from utils.commons.hparams import hparams
    hparams["img2plane_backbone_scale"] = scale
    hparams["img2plane_input_mode"] = mode
    from modules.img2plane.img2plane_model import Img2PlaneModel
    m = Img2PlaneModel(out_channels=96, hp=dict(hparams))          # (without hp the module rebinds its global to a copy of the first call's)
    assert isinstance(m.low_reso_encoder, common.StandInEncoder)
    full = dict(sd)
    full.update({"low_reso_encoder." + k: v for k, v in m.low_reso_encoder.state_dict().items()})
    m.load_state_dict(full, strict=True)
    return m.eval()


def check_from_reference(m, mode, scale):
    """The package's from_reference on the reference's own class: what it reads there (input_mode, hparams, the two num_blocks,
    final_conv.out_channels, low_reso_encoder, the state_dict) is what that class holds, not what a stand-in was given."""
    from real3dportrait_amd.img2plane import Img2PlaneModel as Hip, is_reference_img2plane
    assert is_reference_img2plane(m) and not is_reference_img2plane(m.low_reso_vit)
    hip = Hip.from_reference(m)
    assert hip.low_reso_encoder is m.low_reso_encoder and hip.input_mode == mode == m.input_mode and not hip.training
    assert (hip.low_reso_vit.num_blocks, hip.triplane_predictor_vit.num_blocks) == synth.IMG2PLANE_BLOCKS[scale] \
        == (m.low_reso_vit.num_blocks, m.triplane_predictor_vit.num_blocks)
    assert hip.out_channels == 96 and hip.in_channels == m.high_reso_encoder.first.in_channels
    want, got = m.state_dict(), hip.state_dict()
    assert list(want) != [] and sorted(want) == sorted(got) and all(torch.equal(got[k], v) for k, v in want.items())
    assert not is_reference_img2plane(hip)


@torch.no_grad()
def run(m, x):
    """(planes, taps, the input as assembled): forward hooks on the reference's own modules."""
    got, hooks = {}, []
    keep = lambda name: (lambda mod, inp, out: got.__setitem__(name, out))
    hooks.append(m.low_reso_encoder.register_forward_hook(keep("feat_low")))
    hooks.append(m.low_reso_encoder.register_forward_hook(lambda mod, inp, out: got.__setitem__("x_in", inp[0])))
    hooks.append(m.low_reso_vit.register_forward_hook(keep("feat_low_after_vit")))
    hooks.append(m.high_reso_encoder.register_forward_hook(keep("feat_high")))
    pv = m.triplane_predictor_vit
    hooks.append(getattr(pv, "block%d" % pv.num_blocks).register_forward_hook(keep("tokens")))
    relus = []
    for act in (m.low_reso_vit.activation_conv1, m.low_reso_vit.activation_conv2):
        hooks.append(act.register_forward_hook(lambda mod, inp, out: relus.append(bool((out > 0).any()))))
    planes = m(x)
    for h in hooks:
        h.remove()
    assert relus == [True, True], relus
    t = got.pop("tokens")
    side = int(round(t.shape[1] ** 0.5))
    got["predictor_tokens"] = t.permute(0, 2, 1).reshape(t.shape[0], t.shape[2], side, side)
    return planes, got


def main():
    torch.set_num_threads(16)
    keys = {}
    for name, (mode, scale, S, B, seed_w, seed_x) in common.CASES.items():
        mode, scale, cin, sd, x = common.case_inputs(name)
        m = reference_model(mode, scale, sd)
        check_from_reference(m, mode, scale)
        planes, taps = run(m, torch.from_numpy(x))
        keys.setdefault(mode + "." + scale, np.array(sorted(k for k in m.state_dict() if not k.startswith("low_reso_encoder."))))
        stats = []
        p64, t64 = R64.forward(m.state_dict(), taps["x_in"], taps["feat_low"], torch.float64, stats)
        errs = {"planes": common.rel(p64.numpy(), planes.numpy())}
        errs.update({k: common.rel(t64[k].numpy(), taps[k].numpy()) for k in common.TAPS})
        assert all(e <= common.TOL for e in errs.values()), (name, errs)
        for blk, L, med in stats:
            assert 2.0 / L < med < 0.9, (name, blk, L, med)
        assert all(float(taps[k].abs().max()) > 0 for k in common.TAPS) and float(planes.abs().max()) > 0
        if "alpha" in mode:
            alpha = taps["x_in"][:, 3]
            assert set(np.unique(alpha.numpy()).tolist()) == {0.0, 1.0}
        out = {"spec": np.array([seed_w, seed_x, B, cin, S, S], np.int64), "mode": np.array(mode), "scale": np.array(scale),
               "qk_gain": np.array(common.QK_GAIN), "attention": np.array([[L, med] for _, L, med in stats], np.float64),
               "planes": planes.numpy()}
        for k in common.TAPS:
            out[k] = np.ascontiguousarray(taps[k].numpy()[common.TAP_SLICES[k]])
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **out)
        print("%s: %d bytes, fp64 restatement vs reference %s, attention (L, median max p) %s, max|planes| %.3g"
              % (name, os.path.getsize(path), {k: "%.2g" % v for k, v in errs.items()}, [(L, round(med, 3)) for _, L, med in stats],
                 float(planes.abs().max())))
    # the camera modes' keys: constructed only (no forward)
    for mode in ("rgb_camera", "rgb_alpha_camera"):
        cin = common.MODE_CHANNELS[mode] + 2
        m = reference_model(mode, "small", {k: torch.from_numpy(v) for k, v in synth.synth_img2plane(1, "small", cin).items()})
        check_from_reference(m, mode, "small")
        keys[mode + ".small"] = np.array(sorted(k for k in m.state_dict() if not k.startswith("low_reso_encoder.")))
    np.savez_compressed(os.path.join(HERE, "img2plane_keys.npz"), **keys)


if __name__ == "__main__":
    main()
