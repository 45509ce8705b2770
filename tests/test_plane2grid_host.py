"""CPU: Plane2GridModule's host side (real3dportrait_amd/plane2grid.py, include/r3d_hip_plane2grid.h): the fp64 restatement
against the reference's goldens, state_dict keys, the alpha fold, GroupNorm as scale x + shift, the weight permutation, the header against
its binding table, the argument checks of the r3d_p2g_* entry points, patch_model(plane2grid=True) on mocks, and the golden maker."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import plane2grid_common as common
import plane2grid_ref64 as R64
from abi import C_RETURNS, entry_matches, header_declarations, refusals
from conftest import GOLDEN, ROOT, load_golden

HEADER = "r3d_hip_plane2grid.h"
LLVM = "/opt/rocm/lib/llvm/bin"
NAMES = {"r3d_p2g_groupnorm_stats_workspace_bytes", "r3d_p2g_groupnorm_stats", "r3d_p2g_conv3d"}


@pytest.mark.parametrize("name", list(common.CASES))
def test_fp64_restatement_meets_the_reference(name):
    g = load_golden(name)
    N, D, H, W, alphas, seed_w, seed_x = common.CASES[name]
    D, sd, x = common.case_inputs(name)
    assert [int(v) for v in g["spec"]] == [seed_w, seed_x, N, D, H, W] and [float(a) for a in g["alpha"]] == list(alphas)
    assert g["out"].shape == x.shape and g["conv1"].shape == (3 * N, common.C, D, H, W)
    out, taps = R64.forward(sd, torch.from_numpy(x), D)
    branch = g["out"].astype(np.float64) - x.astype(np.float64)          # the reference's own fp32 branch, recovered
    bmax = float(np.abs(branch).max())
    errs = {"branch": common.rel(taps["branch"].numpy(), branch), "conv1": common.rel(taps["conv1.0"].numpy(), g["conv1"])}
    print(name, errs, "max|y - x| %.3g max|y| %.3g" % (bmax, float(np.abs(g["out"]).max())))
    assert all(e <= common.TOL for e in errs.values()), errs
    assert 1.0 < bmax < 10.0 and bmax < float(np.abs(g["out"]).max())          # the branch is neither negligible nor the whole output


def test_state_dict_keys_are_the_references():
    from real3dportrait_amd.plane2grid import Plane2GridModule
    for D in (1, 2, 3, 4, 6):
        m = Plane2GridModule(D, 96)
        assert m.num_layers_per_block == len(m.res_blocks_3d) == (1 if D <= 3 else 2)
        assert list(m.state_dict()) == common.state_keys(D) == list(common.mock_module(None, D).state_dict())
        shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
        assert shapes["res_blocks_3d.0.conv2.weight"] == (32, 32, 3, 3, 3) and shapes["res_blocks_3d.0.alpha"] == (1,)
        assert shapes["res_blocks_3d.0.norm1.weight"] == shapes["res_blocks_3d.0.conv1.bias"] == (32,)
        assert float(m.res_blocks_3d[0].alpha) == pytest.approx(0.01)
        sd = common.weights(7, D, (0.5, -0.25)[:common.layers_for(D)])
        m.load_state_dict(sd, strict=True)
        assert all(torch.equal(m.state_dict()[k], v) for k, v in sd.items())
        with pytest.raises(RuntimeError):
            m.load_state_dict({k: v for k, v in sd.items() if k != "res_blocks_3d.0.alpha"}, strict=True)
        with pytest.raises(RuntimeError):
            m.load_state_dict(dict(sd, extra=torch.zeros(1)), strict=True)


def test_constructor_and_input_rules():
    from real3dportrait_amd import Plane2GridModule
    from real3dportrait_amd.plane2grid import Plane2GridModule as direct
    assert Plane2GridModule is direct
    for dim in (48, 192, 95):
        with pytest.raises(NotImplementedError, match="in_out_dim = %d" % dim):
            Plane2GridModule(3, dim)
    with pytest.raises(ValueError, match="triplane_depth"):
        Plane2GridModule(0)
    m = Plane2GridModule()
    assert m.triplane_depth == 3 and m.in_out_dim == 96
    with pytest.raises(ValueError, match="not on a GPU"):
        m(torch.zeros(1, 288, 8, 8))
    with pytest.raises(ValueError, match=r"expected \[N, 288, H, W\]"):
        m(torch.zeros(1, 96, 8, 8))
    with pytest.raises(ValueError, match=r"expected \[N, 288, H, W\]"):
        m(torch.zeros(288, 8, 8))
    with pytest.raises(ValueError, match="not float32"):
        m(torch.zeros(1, 288, 8, 8, dtype=torch.float64))
    with pytest.raises(ValueError, match="not contiguous"):
        m.forward_cl(torch.zeros(1, 8, 8, 288).permute(0, 3, 1, 2))


def test_alpha_fold_and_scale_shift_are_the_plain_formulation():
    """x + alpha conv2(relu(gn2(h))) with alpha folded into conv2, and GroupNorm as scale x + shift, against the definitions, in fp64."""
    from real3dportrait_amd.plane2grid import fold_alpha, groupnorm_scale_shift
    torch.manual_seed(0)
    B, C, D, H, W = 3, 32, 2, 5, 4
    x = torch.randn(B, C, D, H, W, dtype=torch.float64) * torch.tensor([0.5, 1.0, 3.0], dtype=torch.float64).view(B, 1, 1, 1, 1) + 0.7
    gamma, beta = 1 + 0.3 * torch.randn(C, dtype=torch.float64), 0.3 * torch.randn(C, dtype=torch.float64)
    scale, shift = groupnorm_scale_shift(x, 4, gamma, beta, 1e-5)
    assert scale.shape == shift.shape == (B, C)
    got = scale.view(B, C, 1, 1, 1) * x + shift.view(B, C, 1, 1, 1)
    want = R64.group_norm(x, gamma, beta)
    assert float((got - want).abs().max()) <= 1e-13 * float(want.abs().max())
    assert float((want - F.group_norm(x, 4, gamma, beta, 1e-5)).abs().max()) <= 1e-13 * float(want.abs().max())
    # a constant group: variance 0 (clamped, never negative), finite scale
    xc = x.clone()
    xc[1, 8:16] = 3.25
    sc, sh = groupnorm_scale_shift(xc, 4, gamma, beta, 1e-5)
    assert bool(torch.isfinite(sc).all()) and bool(torch.isfinite(sh).all())
    assert torch.allclose(sc[1, 8:16], gamma[8:16] / 1e-5 ** 0.5, rtol=1e-9)
    w, b, alpha = torch.randn(C, C, 3, 3, 3, dtype=torch.float64) / 30, torch.randn(C, dtype=torch.float64), torch.tensor([-1.5], dtype=torch.float64)
    h = F.relu(want)
    w2, b2 = fold_alpha(w, b, alpha)
    assert w2.dtype == b2.dtype == torch.float32
    folded = x + R64.conv3d_replicate(h, w.double() * alpha, b.double() * alpha)
    plain = x + alpha * R64.conv3d_replicate(h, w, b)
    assert float((folded - plain).abs().max()) <= 1e-13 * float(plain.abs().max())
    # the fp32 pair is that fold rounded once
    assert torch.equal(w2, (w * alpha).float()) and torch.equal(b2, (b * alpha).float())


def test_weights_are_permuted_depth_major():
    from real3dportrait_amd.plane2grid import conv3d_weight_cl
    w = torch.arange(2 * 4 * 27, dtype=torch.float32).reshape(2, 4, 3, 3, 3)
    p = conv3d_weight_cl(w)
    assert p.shape == (2, 3, 3, 3, 4) and p.is_contiguous()
    for n, kz, ky, kx, c in ((0, 0, 0, 0, 0), (1, 2, 0, 1, 3), (0, 1, 2, 2, 1)):
        assert float(p[n, kz, ky, kx, c]) == float(w[n, c, kz, ky, kx])
    # the kernel's running k = ((kz 3 + ky) 3 + kx) Cin + ci
    assert float(p.reshape(2, -1)[1, ((2 * 3 + 0) * 3 + 1) * 4 + 3]) == float(w[1, 3, 2, 0, 1])


def test_header_mirrors_its_table():
    from real3dportrait_amd import _lib
    lib = _lib.load()
    decls = header_declarations(HEADER)
    assert set(_lib.MODULE_SIGNATURES) == {HEADER}
    table = _lib.MODULE_SIGNATURES[HEADER]
    assert set(decls) == set(table) == NAMES
    others = set(_lib.SIGNATURES) | set(_lib.OPTIONAL_SIGNATURES) | {n for t in _lib.EXTENSION_SIGNATURES.values() for n in t} \
        | {n for t in _lib.FEATURE_SIGNATURES.values() for n in t}
    assert not set(table) & others
    src = open(os.path.join(ROOT, "include", HEADER)).read()
    assert '#include "r3d_hip.h"' in src
    for h in ("r3d_hip.h", "r3d_hip_img2plane.h", "r3d_hip_hubert.h", "r3d_hip_deeplab.h"):
        other = open(os.path.join(ROOT, "include", h)).read()
        assert HEADER not in other and "r3d_p2g_" not in other
    for name, (ret, types) in decls.items():
        res, entries = table[name]
        assert res is C_RETURNS[ret], name
        assert len(entries) == len(types), (name, len(entries), len(types))
        for i, (e, t) in enumerate(zip(entries, types)):
            assert entry_matches(e, t, _lib), "%s: parameter %d is %s in the header, %r in the table" % (name, i, t, e)
        status = res is ctypes.c_int
        # the stream goes last on every status-returning function; the sizer has none
        assert [isinstance(e, _lib.Stream) for e in entries] == [False] * (len(entries) - 1) + [status], name
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == [getattr(e, "ctype", e) for e in entries], name
        assert name in _lib._plans and _lib._plans[name][3] is status
    assert lib.r3d_version() == _lib.ABI_VERSION == 80


@pytest.mark.parametrize("lang", ["c99", "c++17"])
def test_header_stands_alone(lang, tmp_path):
    clang = os.path.join(LLVM, "clang")
    if not os.path.exists(clang):
        pytest.skip("no %s: the header is not compiled here" % clang)
    flags = ["-x", "c", "-std=c99"] if lang == "c99" else ["-x", "c++", "-std=c++17"]
    for i, unit in enumerate(([HEADER], [HEADER, "r3d_hip.h"], ["r3d_hip.h", HEADER], ["r3d_hip_deeplab.h", "r3d_hip_img2plane.h", HEADER, HEADER])):
        src = tmp_path / ("unit%d.%s" % (i, "c" if lang == "c99" else "cpp"))
        src.write_text("".join('#include "%s"\n' % h for h in unit))
        r = subprocess.run([clang] + flags + ["-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                           capture_output=True, text=True)
        assert r.returncode == 0, "%s as %s:\n%s" % (" + ".join(unit), lang, r.stderr)


def test_workspace_bytes():
    from real3dportrait_amd import _lib
    f = _lib.load().r3d_p2g_groupnorm_stats_workspace_bytes
    assert f(3, 3, 256, 256, 32, 4) == 3 * 192 * 4 * 16          # 196 608 rows: 192 blocks of 1024 a sample
    assert f(1, 1, 4, 4, 32, 4) == 64 and f(2, 1, 1025, 1, 32, 8) == 2 * 2 * 8 * 16
    for bad in ((0, 3, 8, 8, 32, 4), (1, 3, 8, 8, 30, 2), (1, 3, 8, 8, 32, 5), (1, 3, 8, 8, 2048, 4), (1, 3, 8, 8, 32, 0), (1 << 16, 1, 1, 1, 32, 4),
                (4, 1024, 128, 128, 32, 4)):
        assert f(*bad) == 0, bad


def test_entry_points_refuse_bad_arguments():
    """Every refusal of the two status-returning r3d_p2g_* entry points: R3D_ERR_INVALID_ARG and a tagged message before any launch (the
    checks run before any HIP call and the addresses are never dereferenced, so they run without a GPU)."""
    from real3dportrait_amd import _lib
    refused = refusals(_lib.load(), "r3d_p2g_")
    X, Y, YN, Wt, Bi, Sc, Sh, R, WS = (0x10000000 * k for k in range(1, 10))
    n = 2 * 3 * 5 * 7          # rows
    cv = dict(x_cl=X, B=2, D=3, H=5, W=7, Cin=32, scale=Sc, shift=Sh, w=Wt, bias=Bi, Cout=32, residual=R, y_cl=Y, y_ncdhw=YN)
    for p in ("x_cl", "w"):
        refused("conv3d", cv, b"NULL pointer", **{p: None})
    refused("conv3d", cv, b"NULL pointer", y_cl=None, y_ncdhw=None)
    refused("conv3d", cv, b"NULL pointer", scale=None)
    refused("conv3d", cv, b"NULL pointer", shift=None)
    for p in ("B", "D", "H", "W", "Cin", "Cout"):
        refused("conv3d", cv, b"bad argument", **{p: 0})
    refused("conv3d", cv, b"bad argument", Cout=4097)
    refused("conv3d", cv, b"bad argument", D=1025)
    for cin in (30, 33, 2):
        refused("conv3d", cv, b"Cin = %d is not a multiple of 4" % cin, Cin=cin)
    refused("conv3d", cv, b"B D H W max(Cin, Cout) = 2147483648 elements, the limit per call is 2^31", B=64, D=4, H=512, W=512)
    refused("conv3d", cv, b"the limit per call is 2^31", B=1, D=1, H=1 << 13, W=1 << 13, Cin=4, Cout=32)
    for p in ("x_cl", "w", "scale", "shift"):
        refused("conv3d", cv, b"not 16-byte aligned", **{p: cv[p] + 4})
    refused("conv3d", cv, b"an output overlaps x, w, bias or the prologue", y_cl=X + 4 * (n * 32 - 1))
    refused("conv3d", cv, b"an output overlaps x, w, bias or the prologue", y_ncdhw=Wt + 4 * (32 * 27 * 32 - 1))
    refused("conv3d", cv, b"an output overlaps x, w, bias or the prologue", bias=Y + 4 * (n * 32 - 1))
    refused("conv3d", cv, b"an output overlaps x, w, bias or the prologue", scale=Y - 16 * (2 * 8 - 1))          # sample 1's row of scale reaches y_cl
    refused("conv3d", cv, b"an output overlaps x, w, bias or the prologue", shift=YN + 16 * (n * 8 - 1))
    refused("conv3d", cv, b"overlaps the residual without y being the residual", residual=Y + 4)
    refused("conv3d", cv, b"overlaps the residual without y being the residual", residual=YN)
    refused("conv3d", cv, b"y and y_ncdhw overlap", y_ncdhw=Y + 4 * (n * 32 - 1))

    gn = dict(x_cl=X, B=2, D=3, H=5, W=7, C=32, groups=4, gamma=Wt, beta=Bi, eps=1e-5, scale=Sc, shift=Sh, workspace=WS, workspace_bytes=2 * 4 * 16)
    for p in ("x_cl", "gamma", "beta", "scale", "shift"):
        refused("groupnorm_stats", gn, b"NULL pointer", **{p: None})
    for p in ("B", "D", "H", "W", "C", "groups"):
        refused("groupnorm_stats", gn, b"bad argument", **{p: 0})
    refused("groupnorm_stats", gn, b"bad argument", B=65536)
    refused("groupnorm_stats", gn, b"C = 30 is not a multiple of 4 and of groups = 2", C=30, groups=2)
    refused("groupnorm_stats", gn, b"C = 32 is not a multiple of 4 and of groups = 5", groups=5)
    refused("groupnorm_stats", gn, b"at most 1024", C=2048)
    for eps in (-1e-5, float("inf"), float("nan")):
        refused("groupnorm_stats", gn, b"is negative or not finite", eps=eps)
    refused("groupnorm_stats", gn, b"the limit per call is 2^31", B=4, D=1024, H=128, W=128)
    refused("groupnorm_stats", gn, b"x_cl is not 16-byte aligned", x_cl=X + 4)
    refused("groupnorm_stats", gn, b"NULL workspace", workspace=None)
    refused("groupnorm_stats", gn, b"the workspace holds 127 bytes, 128 are needed (r3d_p2g_groupnorm_stats_workspace_bytes)", workspace_bytes=127)
    refused("groupnorm_stats", gn, b"the workspace is not 16-byte aligned", workspace=WS + 8)
    refused("groupnorm_stats", gn, b"overlaps another array of the call", shift=Sc + 4 * 63)
    refused("groupnorm_stats", gn, b"overlaps another array of the call", scale=X + 4 * (n * 32 - 1))
    refused("groupnorm_stats", gn, b"overlaps another array of the call", workspace=Sh + 16 * 15)
    refused("groupnorm_stats", gn, b"overlaps another array of the call", gamma=WS + 124)


def mock_model(**modules):
    """The smallest model patch_model accepts, holding `modules` as attributes."""
    class SR(nn.Module):
        def __init__(self):
            super().__init__()
            self.block0 = nn.Linear(1, 1)

    class Model(nn.Module):
        def __init__(self):
            super().__init__()
            self.renderer = nn.Module()
            self.superresolution = SR()
            self.secc_img2plane_backbone = nn.Identity()
            for k, v in modules.items():
                setattr(self, k, v)

    return Model()


def test_from_reference_takes_the_references_layout_only():
    from real3dportrait_amd.plane2grid import Plane2GridModule, is_reference_plane2grid
    sd = common.weights(11, 3, (0.37,))
    mock = common.mock_module(sd, 3)
    assert is_reference_plane2grid(mock) and not is_reference_plane2grid(mock.res_blocks_3d) and not is_reference_plane2grid(nn.Identity())
    hip = Plane2GridModule.from_reference(mock)
    assert type(hip) is Plane2GridModule and not hip.training and not is_reference_plane2grid(hip) and hip.triplane_depth == 3
    assert list(hip.state_dict()) == list(mock.state_dict()) and all(torch.equal(hip.state_dict()[k], v) for k, v in mock.state_dict().items())
    assert len(Plane2GridModule.from_reference(common.mock_module(None, 5)).res_blocks_3d) == 2
    # C != 32 is refused, as is a block that is not the reference's
    for dim in (48, 192):
        assert Plane2GridModule.from_reference(common.mock_module(None, 3, dim)) is None
    odd = common.mock_module(sd, 3)
    odd.res_blocks_3d[0].conv1.padding_mode = "zeros"
    assert Plane2GridModule.from_reference(odd) is None
    odd = common.mock_module(sd, 3)
    odd.res_blocks_3d[0].norm2 = nn.GroupNorm(8, 32)
    assert Plane2GridModule.from_reference(odd) is None
    odd = common.mock_module(sd, 3)
    odd.res_blocks_3d = nn.Sequential(odd.res_blocks_3d[0], common.SameBlock3d(32))
    assert Plane2GridModule.from_reference(odd) is None
    assert Plane2GridModule.from_reference(nn.Identity()) is None
    eps = common.mock_module(sd, 3)
    eps.res_blocks_3d[0].norm1.eps = 1e-3
    assert Plane2GridModule.from_reference(eps).res_blocks_3d[0].norm1.eps == 1e-3


def test_patch_model_swaps_the_module_on_request_only():
    from real3dportrait_amd import Plane2GridModule, patch_model
    import inspect
    params = list(inspect.signature(patch_model).parameters.values())
    assert params[-1].name == "plane2grid" and params[-1].default is False
    sd = common.weights(11, 3, (0.37,))
    old = common.mock_module(sd, 3)
    model = patch_model(mock_model(plane2grid_module=old))
    assert model.plane2grid_module is old and not hasattr(model, "_r3d_reference_plane2grid_module")
    model = patch_model(mock_model(plane2grid_module=old), plane2grid=True)          # without cano_backbone: independent of it
    new = model.plane2grid_module
    assert type(new) is Plane2GridModule and model._r3d_reference_plane2grid_module is old
    assert "_r3d_reference_plane2grid_module" not in dict(model.named_modules()) and "plane2grid_module" in dict(model.named_modules())
    assert all(torch.equal(new.state_dict()[k], v) for k, v in old.state_dict().items())
    assert not any(k.startswith("_r3d_reference") for k in model.state_dict())
    # a model without the attribute, a foreign module and another width are left alone
    model = patch_model(mock_model(), plane2grid=True)
    assert not hasattr(model, "plane2grid_module") and not hasattr(model, "_r3d_reference_plane2grid_module")
    for other in (nn.Identity(), common.mock_module(None, 3, 48)):
        model = patch_model(mock_model(plane2grid_module=other), plane2grid=True)
        assert model.plane2grid_module is other and not hasattr(model, "_r3d_reference_plane2grid_module")
    # patching twice keeps the HIP module and the first reference
    model = patch_model(mock_model(plane2grid_module=old), plane2grid=True)
    first = model.plane2grid_module
    patch_model(model, plane2grid=True)
    assert model.plane2grid_module is first and model._r3d_reference_plane2grid_module is old


def test_golden_maker_reproduces_the_committed_files(tmp_path):
    """A fresh run of tests/golden/make_golden_plane2grid.py (the reference's own class on the CPU) against the committed fixtures."""
    ref = os.environ.get("R3D_REFERENCE", "/root/reference")
    if not os.path.exists(os.path.join(ref, "modules", "real3d", "img2plane_baseline.py")):
        pytest.skip("no reference tree at %s: the goldens cannot be regenerated here" % ref)
    r = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_golden_plane2grid.py"), "--out", str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    for name in common.CASES:
        fresh, stored = dict(np.load(tmp_path / (name + ".npz"))), load_golden(name)
        assert set(fresh) == set(stored) == {"out", "conv1", "spec", "alpha"}
        assert np.array_equal(fresh["spec"], stored["spec"]) and np.array_equal(fresh["alpha"], stored["alpha"])
        for k in ("out", "conv1"):
            # the same program on the same inputs; a CPU conv may sum in another order on another thread count, a few ulp
            assert fresh[k].shape == stored[k].shape and common.rel(fresh[k], stored[k]) <= 1e-6, (name, k, common.rel(fresh[k], stored[k]))
        assert os.path.getsize(os.path.join(GOLDEN, name + ".npz")) < (1 << 20)
