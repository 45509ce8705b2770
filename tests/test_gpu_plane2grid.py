"""GPU: the HIP Plane2GridModule (real3dportrait_amd/plane2grid.py) against the reference's recorded outputs and the fp64
restatement, compared on the branch y - x (the residual x is 5 - 15 times larger and would hide a wrong conv); the two entry points alone
against fp64; bit identities; residual == y; every refusal with real tensors; patch_model(plane2grid=True) in front of the renderer; and
one larger shape against eager fp32 torch on the same GPU."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import plane2grid_common as common
import plane2grid_ref64 as R64
from conftest import load_golden
from real3dportrait_amd import _lib, synth
from test_plane2grid_host import mock_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C, G = common.C, common.GROUPS


@functools.lru_cache(maxsize=None)
def restated(name):
    """The fp64 restatement of a case, computed once: (branch [N, 3 C D, H, W], taps) as numpy."""
    D, sd, x = common.case_inputs(name)
    _, taps = R64.forward(sd, torch.from_numpy(x), D)
    return {k: v.numpy() for k, v in taps.items()}


def cl(t):
    """[B, C, D, H, W] -> channel-last [B, D, H, W, C], contiguous."""
    return t.permute(0, 2, 3, 4, 1).contiguous()


@pytest.mark.parametrize("name", list(common.CASES))
def test_module_meets_the_reference_and_fp64(name):
    g = load_golden(name)
    N, D, H, W = common.CASES[name][:4]
    D, sd, x = common.case_inputs(name)
    m = common.hip_module(sd, D, DEV)
    xt = torch.from_numpy(x).to(DEV)
    out, taps = m._forward_taps(xt)
    assert tuple(out.shape) == x.shape and out.is_contiguous() and out.dtype == torch.float32 and bool(torch.isfinite(out).all())
    assert sorted(taps) == ["conv1.%d" % i for i in range(common.layers_for(D))]
    x64 = x.astype(np.float64)
    branch = out.cpu().numpy().astype(np.float64) - x64
    ref_branch = g["out"].astype(np.float64) - x64          # the reference's own fp32 branch, recovered
    r = restated(name)
    errs = {"branch": common.rel(branch, ref_branch), "conv1": common.rel(taps["conv1.0"].cpu().numpy(), g["conv1"]),
            "branch64": common.rel(branch, r["branch"])}
    errs.update({"%s.64" % k: common.rel(taps[k].cpu().numpy(), r[k]) for k in taps})
    print(name, errs, "max|y - x| %.3g, max|y| %.3g" % (float(np.abs(ref_branch).max()), float(np.abs(g["out"]).max())))
    assert all(e <= common.TOL for e in errs.values()), errs
    # forward_cl is forward, bit for bit, after the permutation; and a second call is the first
    y_cl = m.forward_cl(xt)
    assert tuple(y_cl.shape) == (N, 3, D, H, W, C) and y_cl.is_contiguous()
    assert torch.equal(y_cl.permute(0, 1, 5, 2, 3, 4).reshape(N, 3 * C * D, H, W), out)
    assert torch.equal(m(xt), out)


def stats64(x, gamma, beta, eps=1e-5):
    """(scale, shift) [B, C] in fp64 from the definition (centred variance), x [B, C, D, H, W]."""
    B = x.shape[0]
    g = x.double().reshape(B, G, -1)
    mean = g.mean(dim=2)
    var = ((g - mean.unsqueeze(2)) ** 2).mean(dim=2)
    rstd = (1.0 / torch.sqrt(var + eps)).repeat_interleave(x.shape[1] // G, dim=1)
    scale = gamma.double().view(1, -1) * rstd
    return scale, beta.double().view(1, -1) - mean.repeat_interleave(x.shape[1] // G, dim=1) * scale


def hip_stats(x, gamma, beta, eps=1e-5, groups=G):
    """r3d_p2g_groupnorm_stats on x [B, C, D, H, W] (a CPU tensor): (scale, shift) [B, C] on the device."""
    B, Cx, D, H, W = x.shape
    x_cl = cl(x).to(DEV)
    scale, shift = torch.empty(B, Cx, device=DEV), torch.empty(B, Cx, device=DEV)
    n = _lib.call("r3d_p2g_groupnorm_stats_workspace_bytes", B, D, H, W, Cx, groups)
    ws = torch.empty(n, device=DEV, dtype=torch.uint8)
    _lib.call("r3d_p2g_groupnorm_stats", x_cl, B, D, H, W, Cx, groups, gamma.to(DEV), beta.to(DEV), eps, scale, shift, ws, n)
    return scale, shift


def stats_err(got, want):
    gs, gt = (t.cpu().double() for t in got)
    scale = max(float(want[0].abs().max()), float(want[1].abs().max()))
    return max(float((gs - want[0]).abs().max()), float((gt - want[1]).abs().max())) / scale


@pytest.mark.parametrize("name", list(common.CASES))
def test_statistics_entry_point_at_the_case_shapes(name):
    N, D, H, W = common.CASES[name][:4]
    D, sd, x = common.case_inputs(name)
    xv = torch.from_numpy(x).reshape(3 * N, C, D, H, W)
    gamma, beta = sd["res_blocks_3d.0.norm1.weight"], sd["res_blocks_3d.0.norm1.bias"]
    got = hip_stats(xv, gamma, beta)
    err = stats_err(got, stats64(xv, gamma, beta))
    print(name, "statistics", err)
    assert err <= common.STATS_TOL
    again = hip_stats(xv, gamma, beta)
    assert torch.equal(again[0], got[0]) and torch.equal(again[1], got[1])
    # sample b alone gives sample b's row, bit for bit
    for b in (0, 3 * N - 1):
        one = hip_stats(xv[b:b + 1], gamma, beta)
        assert torch.equal(one[0][0], got[0][b]) and torch.equal(one[1][0], got[1][b])


def test_statistics_of_a_constant_group_an_offset_group_and_many_blocks():
    torch.manual_seed(3)
    # 2 x 30 x 41 = 2460 rows: three blocks a sample, the last one ragged; 64 channels in 8 groups
    x = torch.randn(2, 64, 2, 30, 41)
    x[0, 8:16] = 3.25                                        # constant: variance 0 exactly, no NaN
    x[1, 16:24] = 100.0 + 0.01 * torch.randn(8, 2, 30, 41)   # offset 100, noise 0.01: E[x^2] - mean^2 cancels 8 digits
    gamma, beta = 1 + 0.3 * torch.randn(64), 0.3 * torch.randn(64)
    B, Cx = 2, 64
    x_cl = cl(x).to(DEV)
    scale, shift = torch.empty(B, Cx, device=DEV), torch.empty(B, Cx, device=DEV)
    n = _lib.call("r3d_p2g_groupnorm_stats_workspace_bytes", B, 2, 30, 41, Cx, 8)
    assert n == 2 * 3 * 8 * 16
    ws = torch.empty(n, device=DEV, dtype=torch.uint8)
    _lib.call("r3d_p2g_groupnorm_stats", x_cl, B, 2, 30, 41, Cx, 8, gamma.to(DEV), beta.to(DEV), 1e-5, scale, shift, ws, n)
    assert bool(torch.isfinite(scale).all()) and bool(torch.isfinite(shift).all())
    g = x.double().reshape(B, 8, -1)
    mean = g.mean(dim=2)
    var = ((g - mean.unsqueeze(2)) ** 2).mean(dim=2)
    assert float(var[0, 1]) == 0.0 and 0.5e-4 < float(var[1, 2]) < 2e-4
    rstd = (1.0 / torch.sqrt(var + 1e-5)).repeat_interleave(8, dim=1)
    want_s = gamma.double().view(1, -1) * rstd
    want_t = beta.double().view(1, -1) - mean.repeat_interleave(8, dim=1) * want_s
    # per group, of that group's own magnitude: the constant and the offset group are held to the gate themselves
    for b, gi in ((0, 1), (1, 2), (0, 0), (1, 7)):
        sl = slice(8 * gi, 8 * gi + 8)
        mag = max(float(want_s[b, sl].abs().max()), float(want_t[b, sl].abs().max()))
        err = max(float((scale[b, sl].cpu().double() - want_s[b, sl]).abs().max()), float((shift[b, sl].cpu().double() - want_t[b, sl]).abs().max())) / mag
        print("group", b, gi, err)
        assert err <= common.STATS_TOL, (b, gi, err)
    # the constant group normalises to beta exactly where scale x + shift is formed in fp64
    assert torch.allclose(scale[0, 8:16].cpu().double() * 3.25 + shift[0, 8:16].cpu().double(), beta[8:16].double(), atol=1e-3)


def hip_conv(x, w, b=None, scale=None, shift=None, residual=None, want_cl=False, want_ncdhw=True):
    """r3d_p2g_conv3d on x [B, Cin, D, H, W], w [Cout, Cin, 3, 3, 3] (CPU tensors)."""
    from real3dportrait_amd.plane2grid import conv3d_weight_cl
    B, Cin, D, H, W = x.shape
    Cout = w.shape[0]
    dev = lambda t: None if t is None else t.to(DEV).contiguous()
    y_cl = torch.empty(B, D, H, W, Cout, device=DEV) if want_cl else None
    y_n = torch.empty(B, Cout, D, H, W, device=DEV) if want_ncdhw else None
    _lib.call("r3d_p2g_conv3d", cl(x).to(DEV), B, D, H, W, Cin, dev(scale), dev(shift), conv3d_weight_cl(w).to(DEV), dev(b), Cout,
              None if residual is None else cl(residual).to(DEV), y_cl, y_n)
    return y_cl, y_n


# (B, D, H, W, Cin, Cout): every tile of the table (128 x 32, 32 x 64, 64 x 64, 64 x 16, 128 x 16), ragged M and ragged Cout
CONV_SHAPES = [(2, 2, 5, 7, 32, 32), (1, 3, 6, 5, 8, 40), (1, 2, 128, 128, 4, 40), (1, 1, 9, 4, 12, 12), (1, 2, 128, 128, 4, 8), (3, 1, 1, 1, 4, 20)]


@pytest.mark.parametrize("shape", CONV_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_conv_entry_point_alone(shape):
    """No prologue, no residual, y_ncdhw only, against F.conv3d over F.pad(mode='replicate') in fp64.  The bound is fp32's: every product
    is exact in the fp32 matrix unit's accumulator input and the K + 1 additions round once each, so
    |error| <= (K + 2) 2^-24 (sum |w| |x| + |bias|) element by element, K = 27 Cin."""
    B, D, H, W, Cin, Cout = shape
    torch.manual_seed(sum(shape))
    x, w, b = torch.randn(B, Cin, D, H, W) + 0.5, torch.randn(Cout, Cin, 3, 3, 3) / (27 * Cin) ** 0.5, torch.randn(Cout)
    _, y = hip_conv(x, w, b)
    pad = lambda t: F.pad(t, (1, 1, 1, 1, 1, 1), mode="replicate")
    want = F.conv3d(pad(x.double()), w.double(), b.double())
    bound = (27 * Cin + 2) * 2.0 ** -24 * F.conv3d(pad(x.double().abs()), w.double().abs(), b.double().abs())
    err = (y.cpu().double() - want).abs()
    print(shape, "max error %.3g of max|y| %.3g, largest share of the bound %.3g" % (float(err.max()), float(want.abs().max()), float((err / bound).max())))
    assert bool((err <= bound).all())
    # zero padding instead would not pass: the border differs by far more than the bound (when there is a border to differ at)
    if H > 1:
        zero = F.conv3d(x.double(), w.double(), b.double(), padding=1)
        assert float((zero - want).abs().max()) > 100 * float(bound.max())


def test_conv_prologue_is_per_sample_and_residual_may_be_y():
    """The prologue of a row is its own sample's, in a tile that holds rows of four samples; both outputs hold the same values; and the
    residual may be y_cl itself."""
    from real3dportrait_amd.plane2grid import conv3d_weight_cl
    torch.manual_seed(5)
    B, D, H, W = 4, 1, 5, 5          # 25 rows a sample: one 128-row tile holds all four
    x, w, b = torch.randn(B, C, D, H, W), torch.randn(C, C, 3, 3, 3) / (27 * C) ** 0.5, torch.randn(C)
    scale, shift = 1 + torch.rand(B, C) * torch.arange(1, B + 1).view(B, 1), torch.randn(B, C) * torch.arange(1, B + 1).view(B, 1)
    res = torch.randn(B, C, D, H, W)
    y_cl, y_n = hip_conv(x, w, b, scale, shift, res, want_cl=True)
    assert torch.equal(y_cl.permute(0, 4, 1, 2, 3), y_n)
    act = F.relu(scale.double().view(B, C, 1, 1, 1) * x.double() + shift.double().view(B, C, 1, 1, 1))
    want = F.conv3d(F.pad(act, (1, 1, 1, 1, 1, 1), mode="replicate"), w.double(), b.double()) + res.double()
    assert common.rel(y_n.cpu().numpy(), want.numpy()) <= common.TOL          # the project's gate; a neighbour's (scale, shift) is off by O(1)
    wrong = F.relu(scale.double().roll(1, 0).view(B, C, 1, 1, 1) * x.double() + shift.double().roll(1, 0).view(B, C, 1, 1, 1))
    assert common.rel(F.conv3d(F.pad(wrong, (1, 1, 1, 1, 1, 1), mode="replicate"), w.double(), b.double()).numpy() + res.double().numpy(),
                      want.numpy()) > 0.1
    # each sample alone, with its own row of the prologue: the same bits
    for s in range(B):
        _, one = hip_conv(x[s:s + 1], w, b, scale[s:s + 1], shift[s:s + 1], res[s:s + 1])
        assert torch.equal(one[0], y_n[s]), s
    # residual == y_cl
    inplace = cl(res).to(DEV)
    _lib.call("r3d_p2g_conv3d", cl(x).to(DEV), B, D, H, W, C, scale.to(DEV), shift.to(DEV), conv3d_weight_cl(w).to(DEV), b.to(DEV), C, inplace, inplace,
              None)
    assert torch.equal(inplace, y_cl)


def test_bit_identity_run_to_run_and_sample_wise():
    name = "plane2grid_b_n2_5x7"
    D, sd, x = common.case_inputs(name)
    m = common.hip_module(sd, D, DEV)
    xt = torch.from_numpy(x).to(DEV)
    first = m(xt)          # the work buffers of this shape exist from here on (their factory asks the library for the workspace size)
    with _lib.counting() as calls:
        both = m(xt)
    assert torch.equal(first, both)
    assert [c[0] for c in calls] == ["r3d_torso_volume_to_cl", "r3d_p2g_groupnorm_stats", "r3d_p2g_conv3d", "r3d_p2g_groupnorm_stats", "r3d_p2g_conv3d"]
    assert torch.equal(m(xt), both) and torch.equal(m(xt.clone()), both)
    for n in range(2):
        assert torch.equal(m(xt[n:n + 1].contiguous()), both[n:n + 1]), n
    # two layers: nine launches
    D, sd, x = common.case_inputs("plane2grid_e_d4_8x12")
    m2 = common.hip_module(sd, D, DEV)
    x2 = torch.from_numpy(x).to(DEV)
    m2(x2)
    with _lib.counting() as calls:
        m2(x2)
    assert len(calls) == 9 and [c[0] for c in calls].count("r3d_p2g_conv3d") == 4


def test_parameters_changed_in_place_are_folded_again():
    D, sd, x = common.case_inputs("plane2grid_c_d1_4")
    m = common.hip_module(sd, D, DEV)
    xt = torch.from_numpy(x).to(DEV)
    base = m(xt)
    gen = m._derived.generation
    assert torch.equal(m(xt), base) and m._derived.generation == gen
    with torch.no_grad():
        m.res_blocks_3d[0].alpha.mul_(2.0)
    doubled = m(xt)
    assert m._derived.generation == gen + 1
    # alpha doubled: the branch doubles (a power of two: the folded weights double exactly; the sum x + branch rounds once more)
    b1, b2 = (base - xt).double(), (doubled - xt).double()
    assert float((b2 - 2 * b1).abs().max()) <= 2e-6 * float(doubled.abs().max())
    with torch.no_grad():
        m.res_blocks_3d[0].alpha.zero_()
    assert torch.equal(m(xt), xt)          # alpha 0: weights and bias fold to 0, y = x + 0


def test_every_refusal_leaves_the_outputs_untouched():
    B, D, H, W = 2, 2, 3, 5
    n = B * D * H * W
    x = torch.randn(n * C + 4, device=DEV)
    w, bias, scale, shift = torch.randn(C * 27 * C, device=DEV), torch.randn(C, device=DEV), torch.rand(B * C + 4, device=DEV), torch.randn(B * C, device=DEV)
    res = torch.randn(n * C, device=DEV)
    y, yn = torch.full((n * C + 8,), 7.0, device=DEV), torch.full((n * C,), 7.0, device=DEV)
    base = dict(x_cl=x[:n * C], B=B, D=D, H=H, W=W, Cin=C, scale=scale[:B * C], shift=shift, w=w, bias=bias, Cout=C, residual=res, y_cl=y[:n * C], y_ncdhw=yn)
    p = lambda t, off: t.data_ptr() + 4 * off
    bad = [dict(x_cl=None), dict(w=None), dict(y_cl=None, y_ncdhw=None), dict(scale=None), dict(shift=None), dict(B=0), dict(D=0), dict(H=0), dict(W=0),
           dict(Cin=0), dict(Cout=0), dict(Cin=30), dict(Cin=2), dict(Cout=4097), dict(D=1025), dict(B=1 << 16, H=1 << 5, W=1 << 5),
           dict(x_cl=p(x, 1)), dict(scale=p(scale, 1)), dict(y_cl=p(x, 4)), dict(y_ncdhw=p(w, 0)), dict(y_cl=p(scale, 0)), dict(residual=p(y, 1)),
           dict(residual=p(yn, 0)), dict(y_ncdhw=p(y, 8))]
    for over in bad:
        with pytest.raises(RuntimeError, match="p2g_conv3d failed"):
            _lib.call("r3d_p2g_conv3d", *dict(base, **over).values())
    torch.cuda.synchronize()
    assert bool((y == 7.0).all()) and bool((yn == 7.0).all())
    _lib.call("r3d_p2g_conv3d", *base.values())          # the base call itself is accepted
    assert not bool((y[:n * C] == 7.0).any()) and bool((y[n * C:] == 7.0).all()) and not bool((yn == 7.0).any())

    gamma, beta = torch.randn(C, device=DEV), torch.randn(C, device=DEV)
    so, to = torch.full((B * C,), 7.0, device=DEV), torch.full((B * C + 4,), 7.0, device=DEV)
    nws = _lib.call("r3d_p2g_groupnorm_stats_workspace_bytes", B, D, H, W, C, G)
    ws = torch.full((nws + 16,), 7, device=DEV, dtype=torch.uint8)
    base = dict(x_cl=x[:n * C], B=B, D=D, H=H, W=W, C=C, groups=G, gamma=gamma, beta=beta, eps=1e-5, scale=so, shift=to[:B * C], workspace=ws, workspace_bytes=nws)
    bad = [dict(x_cl=None), dict(gamma=None), dict(beta=None), dict(scale=None), dict(shift=None), dict(workspace=None), dict(B=0), dict(D=0), dict(H=0),
           dict(W=0), dict(C=0), dict(groups=0), dict(groups=3), dict(C=30, groups=2), dict(C=2048), dict(B=65536), dict(eps=-1.0), dict(eps=float("nan")),
           dict(B=4, D=1024, H=128, W=128), dict(x_cl=p(x, 1)), dict(workspace_bytes=nws - 1), dict(workspace=ws.data_ptr() + 8),
           dict(shift=p(so, 1)), dict(scale=p(x, 0)), dict(workspace=so.data_ptr()), dict(gamma=p(to, 0))]
    for over in bad:
        with pytest.raises(RuntimeError, match="p2g_groupnorm_stats failed"):
            _lib.call("r3d_p2g_groupnorm_stats", *dict(base, **over).values())
    torch.cuda.synchronize()
    assert bool((so == 7.0).all()) and bool((to == 7.0).all()) and bool((ws == 7).all())
    _lib.call("r3d_p2g_groupnorm_stats", *base.values())
    assert bool(torch.isfinite(so).all()) and not bool((so == 7.0).any()) and bool((to[B * C:] == 7.0).all()) and bool((ws[nws:] == 7).all())
    # the module's own checks come before the library
    m = common.hip_module(common.weights(11, 3, (0.37,)), 3, DEV)
    for wrong in (torch.zeros(1, 96, 4, 4, device=DEV), torch.zeros(1, 288, 4, 4, device=DEV, dtype=torch.float64),
                  torch.zeros(1, 4, 4, 288, device=DEV).permute(0, 3, 1, 2), torch.zeros(1, 288, 4, 4)):
        with _lib.counting() as calls, pytest.raises(ValueError):
            m(wrong)
        assert calls == []


def test_patch_model_in_front_of_the_renderer():
    """patch_model(plane2grid=True) on a mock, then the package's ImportanceRenderer (trigrid_v2, depth 3) at R = 16 on the installed
    module's grids, against the replaced torch module (eager fp32 on this GPU, a stand-in for the reference) in front of the same renderer."""
    from real3dportrait_amd import ImportanceRenderer, OSGDecoder, Plane2GridModule, RaySampler, patch_model
    name = "plane2grid_a_d3_16"
    D, sd, x = common.case_inputs(name)
    old = common.mock_module(sd, D)
    model = patch_model(mock_model(plane2grid_module=old).to(DEV), plane2grid=True)
    assert type(model.plane2grid_module) is Plane2GridModule and model._r3d_reference_plane2grid_module is old
    assert next(model.plane2grid_module.parameters()).is_cuda
    xt = torch.from_numpy(x).to(DEV)
    with torch.no_grad():
        grids = {"hip": model.plane2grid_module(xt), "torch": model._r3d_reference_plane2grid_module(xt)}
    assert common.rel((grids["hip"] - xt).cpu().numpy(), (grids["torch"] - xt).cpu().numpy()) <= common.TOL
    dec = OSGDecoder(32, {"decoder_lr_mul": 1, "decoder_output_dim": 32}).to(DEV)
    with torch.no_grad():
        for t, v in zip((dec.net[0].weight, dec.net[0].bias, dec.net[2].weight, dec.net[2].bias), synth.synth_decoder(31)):
            t.copy_(torch.from_numpy(np.ascontiguousarray(v)))
    cam = torch.from_numpy(np.asarray(synth.look_at_camera(0.25, 0.1), np.float32)).to(DEV).view(1, 25)
    o, d = RaySampler()(cam[:, :16].view(-1, 4, 4), cam[:, 16:].view(-1, 3, 3), 16)
    opts = {"ray_start": "auto", "ray_end": "auto", "box_warp": 1.0, "depth_resolution": 12, "depth_resolution_importance": 12,
            "disparity_space_sampling": False, "clamp_mode": "softplus", "white_back": False}
    outs = {}
    for k, planes in grids.items():
        ren = ImportanceRenderer(hp={"triplane_feature_type": "trigrid_v2", "triplane_depth": D})
        ren.noise_mode = "hash"
        outs[k] = [t.clone() for t in ren(planes.view(1, 3, C * D, 16, 16), dec, o, d, opts)[:3]]
    for what, a, b in zip(("rgb", "depth", "weights"), outs["hip"], outs["torch"]):
        err = common.rel(a.cpu().numpy(), b.cpu().numpy())
        print("renderer", what, err)
        assert float(b.abs().max()) > 0 and err <= common.TOL, (what, err)
    assert bool(torch.isfinite(outs["hip"][0]).all())


def test_no_torch_conv_runs_in_cal_plane():
    """patch_model(cano_backbone=True, cano_low_reso_encoder=True, plane2grid=True) on a trigrid_v2 mock with the reference's cal_plane
    (img2plane_baseline.py:126-138): no torch convolution or normalisation runs, and the grids are the unpatched mock's within the gate."""
    import deeplabv3_common as dlc
    import img2plane_common as i2p
    from torch.utils._python_dispatch import TorchDispatchMode
    from real3dportrait_amd import patch_model
    D = 3
    bb = i2p.Img2PlaneModel("rgb", "small", out_channels=3 * C * D)
    bb.low_reso_encoder = dlc.DeepLabV3(5)
    sdb = {k: torch.from_numpy(v) for k, v in synth.synth_img2plane(73, "small", 5, qk_gain=i2p.QK_GAIN, out_channels=3 * C * D).items()}
    sdb.update({"low_reso_encoder." + k: v for k, v in dlc.weights(91, 5).items()})
    bb.load_state_dict(sdb, strict=True)
    model = mock_model(img2plane_backbone=bb, plane2grid_module=common.mock_module(common.weights(201, D, (0.37,)), D)).to(DEV).eval()

    def cal_plane(m, img):
        planes = m.img2plane_backbone(img, None)
        b, h, w = planes.shape[0], planes.shape[-2], planes.shape[-1]
        planes = m.plane2grid_module(planes.reshape(b, -1, h, w))
        return planes.reshape(b, 3, -1, h, w)

    img = torch.from_numpy(i2p.image(74, 1, 64)).to(DEV)
    with torch.no_grad():
        want = cal_plane(model, img)
    patch_model(model, cano_backbone=True, cano_low_reso_encoder=True, plane2grid=True)
    cal_plane(model, img)          # buffers and folded weights exist from here on

    class Ops(TorchDispatchMode):
        def __init__(self):
            super().__init__()
            self.seen = []

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            self.seen.append(str(func))
            return func(*args, **(kwargs or {}))
    with _lib.counting() as calls, Ops() as ops:
        got = cal_plane(model, img)
    names = [c[0] for c in calls]
    assert names[-5:] == ["r3d_torso_volume_to_cl", "r3d_p2g_groupnorm_stats", "r3d_p2g_conv3d", "r3d_p2g_groupnorm_stats", "r3d_p2g_conv3d"]
    assert not [o for o in ops.seen if "conv" in o or "norm" in o or "relu" in o], ops.seen
    assert got.shape == want.shape and common.rel(got.cpu().numpy(), want.cpu().numpy()) <= common.TOL


def test_larger_shape_against_eager_torch_on_the_gpu():
    """N = 1, D = 3, 128 x 128 (1152 tiles of 128 rows) against eager fp32 torch of the same module on this GPU.  A STAND-IN, not the
    reference: the mock of tests/plane2grid_common.py with the same weights; the reference's own outputs are the goldens above."""
    D = 3
    sd = common.weights(211, D, (0.37,))
    x = torch.from_numpy(common.planes(212, 1, D, 128, 128)).to(DEV)
    hip, mock = common.hip_module(sd, D, DEV), common.mock_module(sd, D).to(DEV)
    y = hip(x)
    with torch.no_grad():
        ref = mock(x)
    bmax = float((ref - x).abs().max())
    err = float(((y - x) - (ref - x)).abs().max()) / bmax
    print("128 x 128 against eager torch: %.3g of max|y - x| = %.3g" % (err, bmax))
    assert bool(torch.isfinite(y).all()) and err <= common.TOL
