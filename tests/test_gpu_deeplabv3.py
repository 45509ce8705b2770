"""GPU: the HIP DeepLabV3 (real3dportrait_amd/deeplabv3.py) against the reference's recorded outputs and against the same math
in fp32 torch on the GPU; forward against forward_cl; bit-identity of two calls and of a batch against its samples; the staleness rule;
from_reference; Img2PlaneModel's fast path against its generic route; and the library-call counts."""
import numpy as np
import pytest
import torch

import deeplabv3_common as common
import deeplabv3_ref64 as R64
import img2plane_common as i2p
from conftest import load_golden
from real3dportrait_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CALLS = {"resnet34": 46, "resnet18": 30}          # forward_cl: stem 2, two per block + 3 downsamples, ASPP 4 + 4 + 1


@pytest.mark.parametrize("name", list(common.CASES))
def test_module_meets_the_reference(name):
    g = load_golden(name)
    enc, cin, sd, x = common.case_inputs(name)
    m = common.hip_model(sd, cin, DEV, enc)
    xt = torch.from_numpy(x).to(DEV)
    out, taps = m._forward_taps(xt)
    S, B = common.CASES[name][:2]
    assert tuple(out.shape) == (B, 256, S // 8, S // 8) and out.is_contiguous() and bool(torch.isfinite(out).all())
    errs = {"out": common.rel(common.sub(out.cpu().numpy(), common.OUT_BUDGET), g["out"])}
    errs.update({k: common.rel(common.sub(taps[k].cpu().numpy()), g[k]) for k in common.TAPS})
    print(name, errs)
    assert all(e <= common.TOL for e in errs.values()), errs
    if name == "deeplabv3_c_s320":          # the same math in fp32 torch on this GPU, whole tensors
        ref, rtaps = R64.forward({k: v.to(DEV) for k, v in sd.items()}, xt, torch.float32, enc)
        gpu = {"out": common.rel(out.cpu().numpy(), ref.cpu().numpy())}
        gpu.update({k: common.rel(taps[k].cpu().numpy(), rtaps[k].cpu().numpy()) for k in common.TAPS})
        print(name, "against fp32 torch on the GPU", gpu)
        assert all(e <= common.TOL for e in gpu.values()), gpu


def test_forward_is_forward_cl_and_bit_identities():
    name = "deeplabv3_a_s64_b2"
    enc, cin, sd, x = common.case_inputs(name)
    m = common.hip_model(sd, cin, DEV, enc)
    xt = torch.from_numpy(x).to(DEV)
    both = m(xt)
    x_cl = xt.permute(0, 2, 3, 1).contiguous()
    with _lib.counting() as calls:
        y_cl = m.forward_cl(x_cl)
    assert len(calls) == CALLS[enc] and [c[0] for c in calls].count("r3d_dl_conv") == CALLS[enc] - 2
    assert tuple(y_cl.shape) == (2, 8, 8, 256) and torch.equal(y_cl.permute(0, 3, 1, 2), both)
    buf = torch.full((2 * 8 * 8 * 256 + 5,), 3.0, device=DEV)
    y2 = m.forward_cl(x_cl, out=buf)
    assert y2.data_ptr() == buf.data_ptr() and torch.equal(y2, y_cl) and bool((buf[-5:] == 3.0).all())
    with _lib.counting() as calls:
        again = m(xt)
    assert torch.equal(again, both) and len(calls) == CALLS[enc] + 1 and calls[0][0] == "r3d_i2p_nchw_to_cl"
    for b in range(2):
        assert torch.equal(m(xt[b:b + 1].contiguous()), both[b:b + 1]), b


def test_weights_changed_in_place_are_folded_again():
    enc, cin, sd, x = common.case_inputs("deeplabv3_a_s64_b2")
    m = common.hip_model(sd, cin, DEV, enc)
    xt = torch.from_numpy(x[:1]).to(DEV)
    base = m(xt).clone()
    gen = m._derived.generation
    assert torch.equal(m(xt), base) and m._derived.generation == gen
    with torch.no_grad():
        m.decoder[1].weight.mul_(2.0)
    doubled = m(xt)
    assert m._derived.generation == gen + 1 and torch.equal(doubled, 2.0 * base)          # a power of two: exact
    with torch.no_grad():
        m.encoder.layer3[1].bn2.running_var.mul_(4.0)          # a buffer counts too
    assert m._derived.generation == gen + 1 and not torch.equal(m(xt), doubled) and m._derived.generation == gen + 2


def test_from_reference_on_the_mock():
    from real3dportrait_amd.deeplabv3 import DeepLabV3
    name = "deeplabv3_b_s128_c6"
    g = load_golden(name)
    enc, cin, sd, x = common.case_inputs(name)
    mock = common.DeepLabV3(cin, enc)
    mock.load_state_dict(sd, strict=True)
    mock = mock.to(DEV).eval()
    hip = DeepLabV3.from_reference(mock)
    assert type(hip) is DeepLabV3 and next(hip.parameters()).device == torch.device(DEV) and not hip.training
    out = hip(torch.from_numpy(x).to(DEV))
    assert common.rel(common.sub(out.cpu().numpy(), common.OUT_BUDGET), g["out"]) <= common.TOL
    assert common.rel(common.sub(mock(torch.from_numpy(x).to(DEV)).cpu().numpy(), common.OUT_BUDGET), g["out"]) <= common.TOL


@pytest.mark.parametrize("mode", ["rgb", "rgb_alpha_camera"])
def test_backbone_fast_path_is_the_generic_route(mode):
    """Img2PlaneModel over the HIP encoder: r3d_dl_assemble_input + forward_cl against assemble_input + the encoder's NCHW forward over the
    same encoder object, planes bit for bit; no torch convolution runs, and the two layout conversions are gone."""
    from real3dportrait_amd import DeepLabV3, Img2PlaneModel
    cin = i2p.MODE_CHANNELS[mode] + 2
    enc = DeepLabV3(in_channels=cin)
    enc.load_state_dict(common.weights(95, cin), strict=True)
    m = Img2PlaneModel(96, hp={"img2plane_input_mode": mode, "img2plane_backbone_scale": "small"}, low_reso_encoder=enc)
    sd = dict(i2p.weights(73, "small", cin))
    sd.update({"low_reso_encoder." + k: v for k, v in enc.state_dict().items()})
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV).eval()
    S, B = 64, 2
    x = torch.from_numpy(i2p.image(74, B, S, black_rows=S // 4 if "alpha" in mode else 0)).to(DEV)
    cond = {"ref_cameras": torch.from_numpy(common.synth.hash_unitvar(5, (B, 25), 9)).to(DEV)} if "camera" in mode else None
    assert m._fast_encoder() is enc
    m(x, cond)          # buffers and folded weights exist from here on

    class Ops(torch.utils._python_dispatch.TorchDispatchMode):
        def __init__(self):
            super().__init__()
            self.seen = []

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            self.seen.append(str(func))
            return func(*args, **(kwargs or {}))
    with _lib.counting() as calls, Ops() as ops:
        fast, taps = m._forward_taps(x, cond)
    names = [c[0] for c in calls]
    assert len(names) == 1 + CALLS["resnet34"] + 48 and names[0] == "r3d_dl_assemble_input" and "r3d_i2p_nchw_to_cl" not in names
    assert not [o for o in ops.seen if "conv" in o or "batch_norm" in o or "max_pool" in o], ops.seen
    # the input the kernel assembled is the one assemble_input builds, bit for bit
    w = m._buffers_for(x.device, B, S, cin)
    assert torch.equal(w["xcl"].view(B, S, S, cin), m.assemble_input(x, cond).permute(0, 2, 3, 1))
    m._r3d_fast_path = False
    assert m._fast_encoder() is None
    with _lib.counting() as calls:
        generic, gtaps = m._forward_taps(x, cond)
    names = [c[0] for c in calls]
    assert len(names) == (CALLS["resnet34"] + 1) + 50 and names.count("r3d_i2p_nchw_to_cl") == 3 and "r3d_dl_assemble_input" not in names
    assert torch.equal(fast, generic) and bool(torch.isfinite(fast).all()) and float(fast.abs().max()) > 0
    assert sorted(taps) == sorted(gtaps) and all(torch.equal(taps[k], gtaps[k]) for k in taps)
