"""Regenerate the secc_* golden vectors: the reference's SegFormerSECC2PlaneBackbone (modules/real3d/segformer.py:672-731, mode b0) on CPU
in fp32, with the synthetic weights of real3dportrait_amd.synth.synth_secc_backbone and hash inputs.

Run in the build container only (needs the reference tree, R3D_REFERENCE):
    python tests/golden/make_golden_secc.py
Inputs and weights are regenerated from the seeds stored in each file, so the fixtures hold only outputs.

The reference imports timm and mmcv, which are not installed; the stand-ins below provide exactly what the backbone uses: timm's DropPath
(identity in eval), to_2tuple and trunc_normal_ (initialisation only: every parameter is overwritten), and mmcv's ConvModule as
the head builds it (1x1 conv without bias, BatchNorm2d named `bn`, ReLU).  mit_b0.__init__ loads a checkpoint that does not exist here;
torch.load returns {} while the backbone is constructed (load_state_dict(strict=False) of nothing)."""
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

from real3dportrait_amd import synth  # noqa: E402

SEED_W, SEED_X = 11, 12


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
    reg = types.ModuleType("timm.models.registry")
    reg.register_model = lambda f: f
    sys.modules["timm.models.registry"] = reg
    vt = types.ModuleType("timm.models.vision_transformer")
    vt._cfg = lambda **k: k
    sys.modules["timm.models.vision_transformer"] = vt
    cnn = types.ModuleType("mmcv.cnn")

    class ConvModule(nn.Module):
        def __init__(self, in_channels, out_channels, kernel_size, norm_cfg=None, **k):
            super().__init__()
            self.conv = nn.Conv2d(in_channels, out_channels, kernel_size, bias=False)
            self.bn = nn.BatchNorm2d(out_channels)
            self.activate = nn.ReLU()

        def forward(self, x):
            return self.activate(self.bn(self.conv(x)))

    cnn.ConvModule = ConvModule
    sys.modules["mmcv.cnn"] = cnn


def reference_backbone(pncc_cond_mode):
    sys.path.insert(0, HERE)
    _install_stand_ins()
    from modules.real3d.segformer import SegFormerSECC2PlaneBackbone
    load = torch.load
    torch.load = lambda *a, **k: {}
    try:
        m = SegFormerSECC2PlaneBackbone(mode="b0", out_channels=96, pncc_cond_mode=pncc_cond_mode)
    finally:
        torch.load = load
    sd = {k: torch.from_numpy(v) for k, v in synth.synth_secc_backbone(SEED_W, pncc_cond_mode).items()}
    m.load_state_dict(sd, strict=True)
    return m.eval()


def secc_input(seed, B, in_dim, H, W):
    """The driving SECC stack: values in [-1, 1] like the rendered PNCC maps."""
    return synth.hash_uniform(seed, B * in_dim * H * W, stream=5).reshape(B, in_dim, H, W) * np.float32(2.0) - np.float32(1.0)


@torch.no_grad()
def run(m, x):
    t = m.prenet(torch.from_numpy(x))
    feats = m.mix_vit(t)
    head = m.fuse_head(feats)
    return feats, head, m(torch.from_numpy(x))


def main():
    torch.set_num_threads(16)
    for mode, in_dim, tag in (("cano_src_tgt", 9, "a"), ("cano_tgt", 6, "b")):
        m = reference_backbone(mode)
        x = secc_input(SEED_X, 1, in_dim, 64, 64)
        feats, head, planes = run(m, x)
        out = {"spec": np.array([SEED_W, SEED_X, 1, in_dim, 64, 64], np.int64), "mode": np.array(mode)}
        for i, c in enumerate(feats, 1):
            out["c%d" % i] = c.numpy()
        out["head"] = head.numpy()
        out["planes"] = planes.numpy()
        np.savez_compressed(os.path.join(HERE, "secc_%s_r64.npz" % tag), **out)
        print("secc_%s_r64: max|c4| %.3g max|head| %.3g max|planes| %.3g" % (tag, float(feats[3].abs().max()), float(head.abs().max()),
                                                                             float(planes.abs().max())))
    m = reference_backbone("cano_src_tgt")
    x = secc_input(SEED_X + 1, 1, 9, 512, 512)
    with torch.no_grad():
        feats = m.mix_vit(m.prenet(torch.from_numpy(x)))
        head = m.fuse_head(feats)
    np.savez_compressed(os.path.join(HERE, "secc_c_r512.npz"), spec=np.array([SEED_W, SEED_X + 1, 1, 9, 512, 512], np.int64),
                        mode=np.array("cano_src_tgt"), c4=feats[3].numpy(), head_s8=head[:, :, ::8, ::8].numpy())
    print("secc_c_r512: max|c4| %.3g max|head| %.3g" % (float(feats[3].abs().max()), float(head.abs().max())))
    # non-square (H 288, W 256): L = 9 x 8 = 72 keys (one full chunk of 64 plus 8), 72 stage-4 queries, a 72 x 64 head; subsampled to stay
    # under 1 MB
    x = secc_input(SEED_X + 2, 1, 9, 288, 256)
    feats, head, planes = run(m, x)
    np.savez_compressed(os.path.join(HERE, "secc_d_r288x256.npz"), spec=np.array([SEED_W, SEED_X + 2, 1, 9, 288, 256], np.int64),
                        mode=np.array("cano_src_tgt"), c1_s2=feats[0][..., ::2, ::2].numpy(), c2=feats[1].numpy(), c3=feats[2].numpy(),
                        c4=feats[3].numpy(), head_s8=head[..., ::8, ::8].numpy(), planes_s8=planes[..., ::8, ::8].numpy())
    print("secc_d_r288x256: max|c4| %.3g max|head| %.3g max|planes| %.3g" % (float(feats[3].abs().max()), float(head.abs().max()),
                                                                            float(planes.abs().max())))


if __name__ == "__main__":
    main()
