"""GPU parity (`-m gpu`) of the 'f16mx' SR precision (the library default since round 5): f16x3 with the correction products of each 3x3 conv on
the block-scaled 8-bit MFMA (e5m2 activation records x e4m3 weight records).  Own, stated tolerance tier, tighter than the 2e-4 of SURVEY 8(d):
the correction is accurate to e5m2 rounding (~2^-15 of each product), so

    SR outputs   <= 5e-5 * max(1, max|ref|)        (measured 1.6e-5 .. 3.6e-5; f16x3 ~4e-6; TF32 would be ~2e-4)
    final image  <= 2e-4 (SR_TOL) after the clamp

against the same reference goldens, plus the dynamic-range sweep (inputs / weights / styles / biases scaled by 2^k, k in [-20, 14])
at <= 1e-4 * max|ref| vs torch fp64.  The heavy-tail sweeps (tests/test_gpu_pinned_config.py) hold both precisions to SR_TOL near and far."""
import numpy as np
import pytest

from conftest import load_golden
from test_gpu_parity import RGB_TOL, DEPTH_TOL, SR_TOL, T, load_block
from test_gpu_range_and_sizes import SWEEP, _block_fp64, _generator

pytestmark = pytest.mark.gpu
MX_TOL = 5e-5


def test_sr_full_golden_f16mx():
    import torch
    from real3dportrait_amd import SuperresolutionHybrid8XDC, synth
    g = load_golden("sr_full_a")
    seed = int(g["seed"])
    params = synth.synth_sr_params(seed)
    sr = SuperresolutionHybrid8XDC(channels=32, img_resolution=512, sr_num_fp16_res=0, sr_antialias=True).cuda()
    load_block(torch, sr.block0, params[0]); load_block(torch, sr.block1, params[1])
    x = T(torch, synth.hash_unitvar(seed, (1, 32, 128, 128), stream=1))
    ws = torch.ones(1, 14, 512, device="cuda")
    outs = {}
    for prec in ("f16x3", "f16mx"):
        sr.block0.precision = sr.block1.precision = prec
        outs[prec] = sr(x[:, :3].contiguous(), x, ws, noise_mode="none").cpu().numpy()
    out = outs["f16mx"]
    scale = max(1.0, np.abs(g["strided"]).max())
    errs = [np.abs(out[:, :, ::4, ::4] - g["strided"]).max(), np.abs(out[:, :, :96, :96] - g["corner"]).max(),
            np.abs(out[:, :, -64:, -64:] - g["tail"]).max()]
    print("sr_full f16mx max err %.3e (tier %.1e x %.2f); f16x3 %.3e; f16mx vs f16x3 %.3e" %
          (max(errs), MX_TOL, scale, np.abs(outs["f16x3"][:, :, ::4, ::4] - g["strided"]).max(), np.abs(out - outs["f16x3"]).max()))
    assert max(errs) <= MX_TOL * scale
    assert not np.array_equal(out, outs["f16x3"])                     # the fp8 path really ran
    assert abs(float(np.abs(out).mean()) - float(g["absmean"])) <= 1e-4


def test_sr_blocks_golden_f16mx():
    """Two chained blocks with per-layer styles (non-trivial ws) vs the reference's SynthesisBlocks (tests/golden/sr_small_a.npz)."""
    import torch
    from real3dportrait_amd import SynthesisBlock, synth
    g = load_golden("sr_small_a")
    params = synth.synth_sr_params(int(g["seed"]))
    b0 = SynthesisBlock(32, 256, w_dim=512, resolution=32, img_channels=3, is_last=False, conv_clamp=None).cuda()
    b1 = SynthesisBlock(256, 128, w_dim=512, resolution=64, img_channels=3, is_last=True, conv_clamp=None).cuda()
    load_block(torch, b0, params[0]); load_block(torch, b1, params[1])
    b0.precision = b1.precision = "f16mx"
    ws = T(torch, g["ws"])
    x0, r0 = b0(T(torch, g["x"]), T(torch, g["rgb"]), ws, noise_mode="none")
    x1, r1 = b1(x0, r0, ws, noise_mode="none")
    for got, ref in ((x0[:, ::4], g["x0"]), (r0, g["rgb0"]), (x1[:, ::8], g["x1"]), (r1, g["rgb1"])):
        assert np.abs(got.cpu().numpy() - ref).max() <= MX_TOL * max(1.0, np.abs(ref).max())


def test_synthesis_golden_f16mx():
    """TriPlaneGenerator.synthesis (R=128, 48+48, SR -> 512^2) with the SR in f16mx against the reference's output."""
    import torch
    from real3dportrait_amd import synth
    g = load_golden("synthesis_ref_a")
    seed, R, Nc, Nf = int(g["seed"]), int(g["R"]), int(g["Nc"]), int(g["Nf"])
    G = _generator(torch, seed)
    G.superresolution.block0.precision = G.superresolution.block1.precision = "f16mx"
    G.renderer.noise_override = (T(torch, synth.synth_noise(seed, (1, R * R, Nc, 1), stream=7)),
                                 T(torch, synth.synth_noise(seed, (R * R, Nf), stream=8)))
    out = G.synthesis(torch.ones(1, 14, 512, device="cuda"), T(torch, g["cam"]), use_cached_backbone=True, noise_mode="none")
    img = out["image"].cpu().numpy()
    assert np.abs(out["image_raw"].cpu().numpy() - g["image_raw"]).max() <= RGB_TOL
    e_str, e_cor = np.abs(img[:, :, ::4, ::4] - g["image_strided"]).max(), np.abs(img[:, :, :96, :96] - g["image_corner"]).max()
    print("synthesis golden: final image err strided %.2e corner %.2e (tier %.0e x max(1, |ref|))" % (e_str, e_cor, SR_TOL))
    assert e_str <= SR_TOL * max(1.0, np.abs(g["image_strided"]).max()) and e_cor <= SR_TOL * max(1.0, np.abs(g["image_corner"]).max())


@pytest.mark.parametrize("what", ["input", "weights", "styles", "bias"])
@pytest.mark.parametrize("k", SWEEP)
def test_sr_block_range_sweep_f16mx(what, k):
    import torch
    from real3dportrait_amd import synth
    from real3dportrait_amd.superresolution import SynthesisBlock
    N, Cin, Cout, H, W = 2, 32, 128, 18, 14
    sc = np.float32(2.0 ** k)
    p = {kk: tuple(np.array(a) for a in v) for kk, v in synth.synth_sr_block(71, Cin, Cout, 512, 700).items()}
    if what == "weights":
        for layer in ("conv0", "conv1"):
            p[layer] = (p[layer][0] * sc,) + p[layer][1:]
    elif what == "styles":
        for layer in ("conv0", "conv1", "torgb"):
            w_, b_, aw, ab = p[layer]
            p[layer] = (w_, b_, aw * sc, ab * sc)
    elif what == "bias":
        for layer in ("conv0", "conv1"):
            w_, b_, aw, ab = p[layer]
            p[layer] = (w_, b_ * sc, aw, ab)
    blk = SynthesisBlock(Cin, Cout, w_dim=512, resolution=2 * H, img_channels=3, is_last=False, conv_clamp=None).cuda()
    load_block(torch, blk, p)
    blk.precision = "f16mx"
    x = synth.hash_unitvar(72, (N, Cin, H, W), stream=1) * (sc if what == "input" else np.float32(1.0))
    img = synth.hash_unitvar(72, (N, 3, H, W), stream=2) * np.float32(0.5)
    ws = np.ones((N, 3, 512), np.float32) + synth.hash_unitvar(72, (N, 3, 512), stream=3) * np.float32(0.2)
    xo, io = blk(T(torch, x), T(torch, img), T(torch, ws), noise_mode="none")
    rx, ri = _block_fp64(torch, p, torch.from_numpy(x), torch.from_numpy(img), torch.from_numpy(ws), True, None)
    ex = (xo.cpu().double() - rx).abs().max().item() / max(rx.abs().max().item(), 1e-300)
    ei = (io.cpu().double() - ri).abs().max().item() / max(ri.abs().max().item(), 1e-300)
    assert torch.isfinite(xo).all() and torch.isfinite(io).all()
    assert ex <= 1e-4 and ei <= 1e-4, (what, k, ex, ei)


def test_to_plane_stack_f16mx_full_size_batch_equals_singles_and_fp64():
    """to_plane_cnn at its real size (256 ch, 128^2 -> 256^2) under f16mx: a single sample runs the under-filled layers on the 8-row MX tiles
    (conv_mfma_f16x3_rows8_kernel<true>: 256 blocks), a batch of three on the 16x16 MX tiles --
    the same K order per output, so the batch must equal its samples bit for bit; and both stay in the tier against torch fp64."""
    import torch
    from real3dportrait_amd import synth
    from real3dportrait_amd.superresolution import Conv2d, ConvStack, set_sr_precision
    seed, r = 11, 128
    mods, ref_mods = [], []
    for i, ((ci, co, k, lrelu), (w, b)) in enumerate(zip(synth.TO_PLANE_CNN, synth.synth_conv_stack(seed, synth.TO_PLANE_CNN, 500))):
        if i == synth.TO_PLANE_CNN_UP_BEFORE:
            mods.append(torch.nn.UpsamplingBilinear2d(scale_factor=2.)); ref_mods.append(torch.nn.UpsamplingBilinear2d(scale_factor=2.))
        c = Conv2d(ci, co, k, 1, padding=1); rc = torch.nn.Conv2d(ci, co, k, 1, padding=1)
        with torch.no_grad():
            c.weight.copy_(torch.from_numpy(w)); c.bias.copy_(torch.from_numpy(b)); rc.weight.copy_(torch.from_numpy(w)); rc.bias.copy_(torch.from_numpy(b))
        mods.append(c); ref_mods.append(rc)
        if lrelu:
            mods.append(torch.nn.LeakyReLU(0.01)); ref_mods.append(torch.nn.LeakyReLU(0.01))
    cnn = ConvStack(*mods).cuda()
    set_sr_precision(cnn, "f16mx")
    assert all(m.wants_mx() for m in cnn.modules() if isinstance(m, Conv2d))
    x = torch.from_numpy(synth.hash_unitvar(seed, (3, 256, r, r), stream=1)).cuda()
    x[1] *= 0.25; x[2] *= 8.0                                                   # per-sample folds differ
    yb = cnn(x).clone()
    for n in range(3):
        y1 = cnn(x[n:n + 1].contiguous())
        assert torch.equal(y1[0], yb[n]), "sample %d: batch (16x16 MX tiles) != single (8-row MX tiles)" % n
    ref = torch.nn.Sequential(*ref_mods).double()
    with torch.no_grad():
        yr = ref(x[:1].double().cpu())
    e = float((yb[:1].double().cpu() - yr).abs().max() / yr.abs().max())
    print("to_plane_cnn f16mx at 128^2 -> 256^2 vs fp64: %.2e of max|ref|" % e)
    # 2.8e-5 measured.
    assert e <= MX_TOL, e
    convs = [m for m in cnn.modules() if isinstance(m, Conv2d)]
    assert len(convs) == 4


@pytest.mark.parametrize("cout", [128, 96])
def test_conv_up_conv_stack_f16mx_records_from_the_upsampling_step(cout):
    """conv -> UpsamplingBilinear2d(2) -> conv under f16mx: the second conv's operand is one layer from the measured input bound, so the bilinear
    step writes R3D_FMT_SPLIT_MX (fp8 records next to the hi plane) and the conv runs the MX main loop -- also with a padded cout tile (96 -> 128)."""
    import torch
    from real3dportrait_amd import synth
    from real3dportrait_amd.superresolution import Conv2d, ConvStack, set_sr_precision, upsample2x_bilinear
    plan = [(256, 256, 3, True), (256, cout, 3, False)]
    mods, ref_mods = [], []
    for i, ((ci, co, k, lrelu), (w, b)) in enumerate(zip(plan, synth.synth_conv_stack(5, plan, 700))):
        if i == 1:
            mods.append(torch.nn.UpsamplingBilinear2d(scale_factor=2.)); ref_mods.append(torch.nn.UpsamplingBilinear2d(scale_factor=2.))
        c = Conv2d(ci, co, k, 1, padding=1); rc = torch.nn.Conv2d(ci, co, k, 1, padding=1)
        with torch.no_grad():
            c.weight.copy_(torch.from_numpy(w)); c.bias.copy_(torch.from_numpy(b)); rc.weight.copy_(torch.from_numpy(w)); rc.bias.copy_(torch.from_numpy(b))
        mods.append(c); ref_mods.append(rc)
        if lrelu:
            mods.append(torch.nn.LeakyReLU(0.01)); ref_mods.append(torch.nn.LeakyReLU(0.01))
    cnn = ConvStack(*mods).cuda()
    set_sr_precision(cnn, "f16mx")
    seen = []
    import real3dportrait_amd.superresolution as srmod
    orig = srmod.upsample2x_bilinear

    def spy(x, out_format="split", _next=None):
        seen.append(out_format)
        return orig(x, out_format, _next=_next)
    srmod.upsample2x_bilinear = spy
    try:
        x = torch.from_numpy(synth.hash_unitvar(3, (2, 256, 48, 40), stream=1)).cuda()
        y = cnn(x)
    finally:
        srmod.upsample2x_bilinear = orig
    assert seen == ["split_mx"], seen
    with torch.no_grad():
        yr = torch.nn.Sequential(*ref_mods).double()(x.double().cpu())
    e = float((y.double().cpu() - yr).abs().max() / yr.abs().max())
    print("conv -> up -> conv(%d) f16mx vs fp64: %.2e of max|ref|" % (cout, e))
    assert e <= MX_TOL, e
