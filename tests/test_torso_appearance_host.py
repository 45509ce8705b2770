"""CPU: the appearance extractor's host side (real3dportrait_amd/torso_appearance.py, r3d_torso_conv_pool / r3d_torso_conv_split /
r3d_torso_conv3d_res of include/r3d_hip.h).

The fp64 restatement (tests/torso_appearance_ref64.py) against the reference's goldens, the fp64 fold (BatchNorm, the ResBlock3D fold, the
depth-major rows of mid_conv) against the restatement, the state_dict layout against the reference's key list, parameter-version tracking,
the patch_model swap and its guards, argument validation of the C entry points (which runs before any HIP call), the stale-library report
and the kernels' scratch use."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conftest import load_golden
import torso_appearance_ref64 as R64
from torso_motion_ref64 import conv3d
from real3dportrait_amd import synth

GOLDENS = ["appearance_a_r64", "appearance_b_n2_r48x80"]


def T(sd):
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}


def rel(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return float(np.abs(a - ref).max() / np.abs(ref).max())


def golden_case(name):
    """(golden, state_dict, x) -- parameters and the input regenerated from the stored seeds."""
    g = load_golden(name)
    sp, sx, N, in_dim, H, W = (int(v) for v in g["spec"])
    return g, synth.synth_torso_appearance(sp, in_dim), synth.synth_torso_appearance_inputs(sx, N, in_dim, H, W)["x"]


def subsample(g, out):
    """The golden's depth stride applied to a full output (tests/golden/make_golden_torso_appearance.py)."""
    return out[:, :, ::int(g["strides"][0])]


def hip_extractor(sd, in_dim, precision="f32"):
    from real3dportrait_amd.torso_appearance import AppearanceFeatureExtractor
    m = AppearanceFeatureExtractor(in_dim=in_dim, precision=precision)
    m.load_state_dict(T(sd), strict=True)
    return m.eval()


def reference_like_extractor(seed=5, in_dim=5, n_res=6):
    """A stand-in for the reference's AppearanceFeatureExtractor in plain torch, with its class name, attributes and state_dict keys, built
    by the reference's layer recipe (layers.py; BatchNorm for SyncBatchNorm, which evaluates the same in eval mode).  Its forward is the
    restatement in float32 on its own state_dict."""
    def block(dim, pattern, ci, co, k):
        conv, norm = (nn.Conv2d, nn.BatchNorm2d) if dim == 2 else (nn.Conv3d, nn.BatchNorm3d)
        mods = {"C": conv(ci, co, k, 1, k // 2), "N": norm(co if pattern[0] == "C" else ci), "A": nn.ReLU(inplace=True)}
        m = nn.Module()
        m.layers = nn.Sequential(*[mods[c] for c in pattern])
        return m

    def wrap(*mods):
        m = nn.Module()
        m.layers = nn.Sequential(*mods)
        return m

    class AppearanceFeatureExtractor(nn.Module):
        def __init__(self):
            super().__init__()
            self.in_conv = block(2, "CNA", in_dim, 64, 7)
            self.down = nn.Sequential(*[wrap(block(2, "CNA", ci, co, 3), nn.AvgPool2d((2, 2))) for ci, co in ((64, 128), (128, 256))])
            self.mid_conv = nn.Conv2d(256, 32 * 16, 1, 1, 0)
            self.res = nn.Sequential(*[wrap(block(3, "NAC", 32, 32, 3), block(3, "NAC", 32, 32, 3)) for _ in range(n_res)])
            self.C, self.D = 32, 16

        @torch.no_grad()
        def forward(self, x):
            return R64.extractor(self.state_dict(), x, dtype=torch.float32)

    m = AppearanceFeatureExtractor().eval()
    if n_res == 6:
        m.load_state_dict(T(synth.synth_torso_appearance(seed, in_dim)), strict=True)
    return m


def run_folded(Fd, x):
    """fold_appearance's layers as the kernels evaluate them, in fp64 torch: conv + bias + ReLU (+ pool), mid_conv with depth-major rows
    stored as [N, 16, H, W, 32], the prologue applied before the zero padding, the residual after the activation."""
    cw2, cw3 = (lambda w: w.permute(0, 3, 1, 2)), (lambda w: w.permute(0, 4, 1, 2, 3))
    L = Fd["in_conv"]
    x = F.relu(F.conv2d(x, cw2(L["w"]), L["b"], padding=3))
    for L in Fd["down"]:
        x = F.avg_pool2d(F.relu(F.conv2d(x, cw2(L["w"]), L["b"], padding=1)), (2, 2))
    y = F.conv2d(x, cw2(Fd["mid"]["w"]), Fd["mid"]["b"])                # channel d 32 + c
    N, _, H, W = y.shape
    x = y.view(N, 16, 32, H, W).permute(0, 2, 1, 3, 4)                  # -> [N, c, d, H, W]
    res_in = None
    for L in Fd["res"]:
        a = x
        if L["ps"] is not None:
            a = F.relu(a * L["ps"][None, :, None, None, None] + L["pt"][None, :, None, None, None])
            res_in = x
        y = conv3d(a, cw3(L["w"]), L["b"], 1)
        if L["act"] == 1:
            y = F.relu(y)
        x = y + res_in if L["res"] else y
    return x


def test_state_dict_keys_are_the_reference_s():
    keys = [str(k) for k in load_golden("appearance_keys")["extractor"]]
    for in_dim, lo, hi in ((3, 0.8435e6, 0.8445e6), (5, 0.8495e6, 0.8505e6)):
        m = hip_extractor(synth.synth_torso_appearance(1, in_dim), in_dim)
        assert list(m.state_dict().keys()) == keys and len(keys) == 107
        shapes = dict(synth.torso_appearance_shapes(in_dim))
        assert list(shapes) == keys
        for k, v in m.state_dict().items():
            assert tuple(v.shape) == tuple(shapes[k]), k
        assert lo < sum(int(np.prod(p.shape)) for p in m.parameters()) < hi


def test_strict_load_from_a_reference_like_module():
    from real3dportrait_amd.torso_appearance import AppearanceFeatureExtractor, is_reference_appearance_extractor
    import real3dportrait_amd
    assert real3dportrait_amd.TorsoAppearanceFeatureExtractor is AppearanceFeatureExtractor
    ref = reference_like_extractor(5, 5)
    assert is_reference_appearance_extractor(ref) and not is_reference_appearance_extractor(reference_like_extractor(n_res=4))
    assert not is_reference_appearance_extractor(nn.Conv2d(1, 1, 1)) and not is_reference_appearance_extractor(None)
    m = AppearanceFeatureExtractor.from_reference(ref)
    assert not is_reference_appearance_extractor(m) and m.in_dim == 5 and m.precision == "f32"
    assert AppearanceFeatureExtractor.from_reference(ref, "bf16x3").precision == "bf16x3"
    for k, v in ref.state_dict().items():
        assert torch.equal(m.state_dict()[k], v) and m.state_dict()[k].dtype == v.dtype, k
    sd = T(synth.synth_torso_appearance(5, 3))
    for missing in ("in_conv.layers.1.running_var", "down.1.layers.0.layers.0.bias", "mid_conv.weight", "res.5.layers.1.layers.0.running_mean",
                    "res.0.layers.0.layers.2.weight"):
        with pytest.raises(RuntimeError, match="Missing key"):
            AppearanceFeatureExtractor().load_state_dict({k: v for k, v in sd.items() if k != missing}, strict=True)
    with pytest.raises(RuntimeError, match="Unexpected key"):
        AppearanceFeatureExtractor().load_state_dict(dict(sd, extra=torch.zeros(1)), strict=True)


def test_guards():
    from real3dportrait_amd import patch_model
    from real3dportrait_amd.torso_appearance import AppearanceFeatureExtractor
    from test_torso_generator_host import model_shell, reference_like_torso_model
    with pytest.raises(NotImplementedError, match="lora_args"):
        AppearanceFeatureExtractor(lora_args={"rank": 4})
    for bad in ("bf16", "F32", None, 1):
        with pytest.raises(ValueError):
            AppearanceFeatureExtractor(precision=bad)
    m = AppearanceFeatureExtractor(in_dim=5)
    for shape in ((1, 3, 64, 64), (1, 5, 62, 64), (1, 5, 64, 66), (1, 5, 0, 64), (5, 64, 64)):
        with pytest.raises(ValueError):
            m(torch.zeros(*shape))
    with pytest.raises(ValueError, match="torso_appearance"):
        patch_model(model_shell(reference_like_torso_model()), torso_precision="bf16x3")         # without any torso switch
    with pytest.raises(ValueError):
        patch_model(model_shell(reference_like_torso_model()), torso_appearance=True, torso_precision="fp16")
    for given, want in ((None, "f32"), ("f32", "f32"), ("bf16x3", "bf16x3")):
        tm = reference_like_torso_model()
        tm.appearance_extractor = reference_like_extractor()
        patch_model(model_shell(tm), torso_appearance=True, torso_precision=given)
        assert tm.appearance_extractor.precision == want


@pytest.mark.parametrize("name", GOLDENS)
def test_fp64_restatement_matches_reference_goldens(name):
    torch.set_num_threads(8)
    g, sd, x = golden_case(name)
    with torch.no_grad():
        out = R64.extractor(sd, torch.from_numpy(x))
    e = rel(subsample(g, out).numpy(), g["out"])
    print(name, e)
    assert e <= 1e-4, e
    if x.shape[0] > 1:
        assert not np.array_equal(g["out"][0], g["out"][1])


def test_fp64_fold_equals_the_fp64_restatement():
    """The BatchNorm of every "CNA" conv folded into weight and bias, the ResBlock3D fold (BN1 + ReLU as prologue, BN2 + ReLU in conv A's
    rows, bias and epilogue, conv B plain plus the residual) and the depth-major order of mid_conv's rows."""
    from real3dportrait_amd.torso_appearance import fold_appearance
    torch.set_num_threads(8)
    sd = synth.synth_torso_appearance(7, 5)
    x = torch.from_numpy(synth.synth_torso_appearance_inputs(8, 2, 5, 24, 40)["x"]).double()
    with torch.no_grad():
        ref = R64.extractor(sd, x)
        Fd = fold_appearance(hip_extractor(sd, 5), torch.float64)
        assert all(l["w"].dtype == torch.float64 for l in Fd["down"] + Fd["res"] + [Fd["in_conv"], Fd["mid"]])
        assert Fd["in_conv"]["w"].shape == (64, 7, 7, 5) and Fd["down"][1]["w"].shape == (256, 3, 3, 128)
        assert Fd["mid"]["w"].shape == (512, 1, 1, 256) and Fd["res"][0]["w"].shape == (32, 3, 3, 3, 32) and len(Fd["res"]) == 12
        mw = torch.from_numpy(sd["mid_conv.weight"]).double()
        assert torch.equal(Fd["mid"]["w"][3 * 32 + 7, 0, 0], mw[7 * 16 + 3, :, 0, 0])            # row d 32 + c = channel c 16 + d
        assert float(Fd["mid"]["b"][3 * 32 + 7]) == float(sd["mid_conv.bias"][7 * 16 + 3])
        out = run_folded(Fd, x)
    e = rel(out.numpy(), ref.numpy())
    print("fold vs restatement:", e)
    assert e <= 1e-12, e


def test_in_place_parameter_edits_are_seen_by_the_next_prepare():
    m = hip_extractor(synth.synth_torso_appearance(5, 3), 3)
    a = m._prepare()
    assert m._prepare() is a
    w0 = a["down"][1]["w"].clone()
    with torch.no_grad():
        m.down[1].layers[0].layers[0].weight.add_(0.01)
    b = m._prepare()
    assert b is not a and not torch.equal(b["down"][1]["w"], w0) and torch.equal(b["down"][0]["w"], a["down"][0]["w"])
    with torch.no_grad():
        m.res[2].layers[0].layers[0].running_var.mul_(2.0)
    c = m._prepare()
    assert c is not b and not torch.equal(c["res"][4]["ps"], b["res"][4]["ps"]) and torch.equal(c["res"][2]["ps"], b["res"][2]["ps"])
    with torch.no_grad():
        m.mid_conv.bias.add_(1.0)
    d = m._prepare()
    assert d is not c and float(d["mid"]["b"][5] - c["mid"]["b"][5]) == pytest.approx(1.0, abs=1e-6)
    # a parameter replaced by another tensor at the same address and version (what the caching allocator makes of a freed one)
    from test_state_host import replaced_at_same_address
    e, f = replaced_at_same_address(m.down[1].layers[0].layers[0], "weight", m._prepare)
    assert f is not e and not torch.equal(f["down"][1]["w"], e["down"][1]["w"]) and torch.equal(f["down"][0]["w"], e["down"][0]["w"])
    assert m._prepare() is f


def test_patch_model_swaps_the_extractor_only_with_the_flag():
    from real3dportrait_amd import patch_model, TorsoAppearanceFeatureExtractor
    from test_torso_generator_host import model_shell, reference_like_torso_model
    ext = reference_like_extractor(5, 5)
    tm = reference_like_torso_model()
    tm.appearance_extractor = ext
    gen = tm.deform_based_generator
    patch_model(model_shell(tm))
    assert tm.appearance_extractor is ext
    patch_model(model_shell(tm), torso_generator=True, torso_motion=True, torso_appearance=False)
    assert tm.appearance_extractor is ext
    tm.deform_based_generator = gen
    before = {k: v.clone() for k, v in tm.appearance_extractor.state_dict().items()}
    patch_model(model_shell(tm), torso_appearance=True)
    assert isinstance(tm.appearance_extractor, TorsoAppearanceFeatureExtractor) and tm.deform_based_generator is gen
    after = tm.appearance_extractor.state_dict()
    assert list(after) == list(before)
    for k, v in before.items():
        assert after[k].dtype == v.dtype and torch.equal(after[k], v), k


def test_patch_model_leaves_foreign_modules_alone():
    from real3dportrait_amd import patch_model
    from test_torso_generator_host import model_shell, reference_like_torso_model
    tm = reference_like_torso_model()
    other = reference_like_extractor(n_res=4)                  # the class name, another architecture
    tm.appearance_extractor = other
    patch_model(model_shell(tm), torso_appearance=True)
    assert tm.appearance_extractor is other
    tm.appearance_extractor = nn.Conv2d(1, 1, 1)
    patch_model(model_shell(tm), torso_appearance=True)
    assert type(tm.appearance_extractor) is nn.Conv2d
    del tm.appearance_extractor
    patch_model(model_shell(tm), torso_appearance=True)        # no extractor at all
    assert not hasattr(tm, "appearance_extractor")


def test_c_entry_points_reject_bad_arguments_without_a_gpu():
    from real3dportrait_amd import _lib
    lib = _lib.load()
    assert lib.r3d_version() == _lib.ABI_VERSION
    at = lambda i: ctypes.c_void_p((1 << 30) + 4 * i)       # never dereferenced: validation fails first
    far, far2, far3, far4 = (ctypes.c_void_p(1 << s) for s in (40, 41, 42, 43))
    err = lambda: lib.r3d_last_error()

    def pool(x, w, y, B=1, H=8, W=8, Cin=32, nchw=0, Cout=64, k=3, act=1, pool=1, prec=0):
        return lib.r3d_torso_conv_pool(x, B, H, W, Cin, nchw, w, None, Cout, k, act, 0.0, pool, y, prec, None)

    assert pool(None, far, far2) == -1 and b"NULL" in err()
    assert pool(at(0), None, far2) == -1 and b"NULL" in err()
    assert pool(at(0), far, None) == -1 and b"NULL" in err()
    assert pool(at(0), far, far2, H=7) == -1 and b"odd size" in err()
    assert pool(at(0), far, far2, W=5) == -1 and b"odd size" in err()
    assert pool(at(0), far, far2, pool=2) == -1 and b"pool 2" in err()
    assert pool(at(0), far, far2, k=5) == -1 and b"ksize 5" in err()
    assert pool(at(0), far, far2, act=3) == -1 and b"act 3" in err()
    assert pool(at(0), far, far2, Cin=0) == -1 and b"bad argument" in err()
    assert pool(at(0), far, far2, Cout=5000) == -1 and b"bad argument" in err()
    assert pool(at(0), far, far2, prec=2) == -1 and b"precision 2" in err()
    assert pool(at(0), far, far2, prec=-1) == -1 and b"precision -1" in err()
    # x [1, 8, 8, 32] = 2048 floats; the pooled y [1, 4, 4, 64] = 1024, the un-pooled one 4096
    assert pool(at(0), far, at(2047)) == -1 and b"overlaps x" in err()
    assert pool(at(1023), far, at(0)) == -1 and b"overlaps x" in err()
    assert pool(at(4095), far, at(0), pool=0) == -1 and b"overlaps x" in err()
    assert pool(at(100000), at(0), at(64 * 9 * 32 - 1)) == -1 and b"overlaps x, w" in err()

    def split(x, w, y, B=1, H=8, W=8, Cin=32, Cout=64, k=1, depth=16, prec=0):
        return lib.r3d_torso_conv_split(x, B, H, W, Cin, 0, w, None, Cout, k, 0, 0.0, depth, y, prec, None)

    assert split(None, far, far2) == -1 and b"NULL" in err()
    assert split(at(0), far, None) == -1 and b"NULL" in err()
    assert split(at(0), far, far2, Cout=65) == -1 and b"not a multiple" in err()
    assert split(at(0), far, far2, depth=48) == -1 and b"not a multiple" in err()
    assert split(at(0), far, far2, depth=0) == -1 and b"not a multiple" in err()
    assert split(at(0), far, far2, depth=-2) == -1 and b"not a multiple" in err()
    assert split(at(0), far, far2, H=0) == -1 and b"bad argument" in err()
    assert split(at(0), far, far2, prec=7) == -1 and b"precision 7" in err()
    assert split(at(0), far, at(2047)) == -1 and b"overlaps x" in err()
    assert split(at(4095), far, at(0)) == -1 and b"overlaps x" in err()

    def res(x, w, y, yn=None, r=None, ps=None, pt=None, B=1, D=4, H=8, W=8, Cin=32, Cout=32, k=3, act=0, prec=0):
        return lib.r3d_torso_conv3d_res(x, B, D, H, W, Cin, ps, pt, 0.0, w, None, Cout, k, act, 0.0, r, y, yn, prec, None)

    assert res(None, far, far2) == -1 and b"NULL" in err()
    assert res(at(0), None, far2) == -1 and b"NULL" in err()
    assert res(at(0), far, None) == -1 and b"NULL" in err()                        # no output at all
    assert res(at(0), far, far2, ps=far3) == -1 and b"NULL" in err()               # half a prologue
    assert res(at(0), far, far2, pt=far3) == -1 and b"NULL" in err()
    assert res(at(0), far, far2, D=0) == -1 and b"bad argument" in err()
    assert res(at(0), far, far2, D=2000) == -1 and b"bad argument" in err()
    assert res(at(0), far, far2, k=2) == -1 and b"ksize 2" in err()
    assert res(at(0), far, far2, act=-1) == -1 and b"act -1" in err()
    assert res(at(0), far, far2, prec=3) == -1 and b"precision 3" in err()
    # x, y, y_ncdhw and the residual [1, 4, 8, 8, 32] = 8192 floats each
    assert res(at(0), far, at(8191)) == -1 and b"overlaps x" in err()
    assert res(at(100000), far, None, at(99999)) == -1 and b"overlaps x" in err()
    assert res(at(100000), far, at(0), at(8191)) == -1 and b"y and y_ncdhw" in err()
    assert res(at(100000), far, at(0), r=at(8191)) == -1 and b"overlaps the residual" in err()
    assert res(at(100000), far, at(0), at(20000), r=at(20001)) == -1 and b"overlaps the residual" in err()
    assert res(at(100000), far, at(0), ps=at(8191), pt=far4) == -1 and b"prologue" in err()
    assert res(at(100000), at(0), at(32 * 27 * 32 - 1)) == -1 and b"overlaps x, w" in err()


def test_load_reports_a_library_without_the_new_symbols_as_stale(monkeypatch):
    """The three functions arrive without a new ABI number, so a library built before them passes the version check: load() must name the
    missing symbol and say to rebuild."""
    from real3dportrait_amd import _lib
    lib = _lib.load()
    for name in ("r3d_torso_conv_pool", "r3d_torso_conv_split", "r3d_torso_conv3d_res"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)

    class Stale:                                               # what ctypes gives for a library built before this module
        def __init__(self, real, missing):
            self._real, self._missing = real, missing

        def __getattr__(self, name):
            if name == self._missing:
                raise AttributeError(name)
            return getattr(self._real, name)

    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(ctypes, "CDLL", lambda *a, **k: Stale(lib, "r3d_torso_conv3d_res"))
    with pytest.raises(RuntimeError, match="does not export r3d_torso_conv3d_res.*rebuild"):
        _lib.load()
    assert _lib._lib is None


def test_appearance_kernels_do_not_use_scratch():
    from test_render_kernel_resources import _kernel_metadata
    from real3dportrait_amd import _lib
    meta = _kernel_metadata(_lib.LIB_PATH)
    names = [k for k in meta if "tappear" in k]
    assert len(names) == 20, names          # conv x (5 tiles x 2 loaders x 2 tiers)
    for k in names:
        assert int(meta[k]["private_segment_fixed_size"]) == 0, (k, meta[k])
        assert int(meta[k]["vgpr_spill_count"]) == 0, (k, meta[k])
