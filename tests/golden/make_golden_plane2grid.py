"""Regenerate the plane2grid_* golden vectors: the reference's Plane2GridModule (modules/real3d/img2plane_baseline.py:58-77) on CPU in fp32,
its own __init__ and forward, with the synthetic weights and inputs of tests/plane2grid_common.py.

Run in the build container only (needs the reference tree, R3D_REFERENCE):
    python tests/golden/make_golden_plane2grid.py [--out DIR]
Inputs and weights are regenerated from the seeds of plane2grid_common.CASES, so the fixtures hold only outputs.

img2plane_baseline.py imports the whole model (segformer, eg3d, the torso network), whose imports timm, mmcv, torchvision and others are not
installed: ref_stubs.install() plus the stand-ins of make_golden_secc.py (DropPath, to_2tuple, trunc_normal_, register_model, _cfg,
ConvModule) go into sys.modules first.  Nothing on the path of Plane2GridModule calls into them; einops is installed and is the real one.

Stored per case: `out` [N, 3 C D, H, W], the module's output; `conv1` [3N, C, D, H, W], the output of layer 0's conv1, captured with a forward
hook; `spec` = (weight seed, input seed, N, D, H, W); `alpha`.  The maker requires the fp64 restatement (tests/plane2grid_ref64.py) to meet
the reference within 2e-4 of max|y_ref - x| on the branch y - x and of max|tap| on conv1, and runs the package's
Plane2GridModule.from_reference on the reference's own class."""
import argparse
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

import plane2grid_common as common  # noqa: E402
import plane2grid_ref64 as R64  # noqa: E402


def _install_stand_ins():
    import ref_stubs
    ref_stubs.install()
    layers = types.ModuleType("timm.models.layers")

    class DropPath(nn.Module):
        def __init__(self, p=0.0):
            super().__init__()

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
        def __init__(self, *a, **k):
            super().__init__()

    cnn.ConvModule = ConvModule
    sys.modules["mmcv.cnn"] = cnn
    # the reference's DeepLabV3 package imports pretrainedmodels and torchvision's ResNet: never imported, as in make_golden_img2plane.py
    deeplab = types.ModuleType("modules.img2plane.deeplabv3")
    deeplab.DeepLabV3 = nn.Identity
    sys.modules["modules.img2plane.deeplabv3"] = deeplab


def reference_module(depth, sd):
    _install_stand_ins()
    from modules.real3d.img2plane_baseline import Plane2GridModule
    m = Plane2GridModule(triplane_depth=depth, in_out_dim=3 * common.C)
    assert list(m.state_dict()) == common.state_keys(depth), list(m.state_dict())
    m.load_state_dict(sd, strict=True)
    return m.eval()


def check_from_reference(m):
    from real3dportrait_amd.plane2grid import Plane2GridModule as Hip, is_reference_plane2grid
    assert is_reference_plane2grid(m) and not is_reference_plane2grid(m.res_blocks_3d)
    hip = Hip.from_reference(m)
    assert type(hip) is Hip and hip.triplane_depth == m.triplane_depth and not hip.training and not is_reference_plane2grid(hip)
    want, got = m.state_dict(), hip.state_dict()
    assert list(want) == list(got) and all(torch.equal(got[k], v) for k, v in want.items())
    assert [(b.norm1.eps, b.norm2.eps) for b in hip.res_blocks_3d] == [(b.norm1.eps, b.norm2.eps) for b in m.res_blocks_3d]


@torch.no_grad()
def run(m, x):
    got = {}
    h = m.res_blocks_3d[0].conv1.register_forward_hook(lambda mod, inp, out: got.__setitem__("conv1", out))
    out = m(x)
    h.remove()
    return out, got["conv1"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    out_dir = ap.parse_args().out
    torch.set_num_threads(8)
    for name, (N, D, H, W, alphas, seed_w, seed_x) in common.CASES.items():
        D, sd, x = common.case_inputs(name)
        m = reference_module(D, sd)
        check_from_reference(m)
        xt = torch.from_numpy(x)
        out, conv1 = run(m, xt)
        assert tuple(out.shape) == tuple(x.shape) and tuple(conv1.shape) == (3 * N, common.C, D, H, W)
        o64, t64 = R64.forward(sd, xt, D)
        branch = out.double() - xt.double()
        bmax = float(branch.abs().max())
        errs = {"branch": float((branch - t64["branch"]).abs().max()) / bmax, "conv1": common.rel(conv1.numpy(), t64["conv1.0"].numpy())}
        assert all(e <= common.TOL for e in errs.values()), (name, errs)
        path = os.path.join(out_dir, name + ".npz")
        np.savez_compressed(path, out=out.numpy(), conv1=conv1.numpy(), spec=np.array([seed_w, seed_x, N, D, H, W], np.int64),
                            alpha=np.array(alphas, np.float64))
        print("%s: %d bytes, reference vs fp64 restatement %s, max|y - x| %.3g, max|y| %.3g, max|conv1| %.3g"
              % (name, os.path.getsize(path), {k: "%.2g" % v for k, v in errs.items()}, bmax, float(out.abs().max()), float(conv1.abs().max())))


if __name__ == "__main__":
    main()
