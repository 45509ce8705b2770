"""GPU: the HIP Img2PlaneModel (real3dportrait_amd/img2plane.py) end to end against the reference's own outputs
(tests/golden/img2plane_*.npz, made by tests/golden/make_golden_img2plane.py): the planes and four taps within 2e-4 of max|ref|;
loading from a state_dict the way from_reference does; patch_model(cano_backbone=True); bit-identity of two calls and of a batch
against its samples."""
import numpy as np
import pytest
import torch

import img2plane_common as common
from test_img2plane_host import mock_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("name", list(common.CASES))
def test_goldens(name):
    g, mode, scale, cin, sd, x = common.golden_case(name)
    m = common.hip_model(mode, scale, sd, DEV)
    planes, taps = m._forward_taps(torch.from_numpy(x).to(DEV))
    assert planes.shape == g["planes"].shape and planes.is_contiguous() and planes.dtype == torch.float32
    errs = {"planes": common.rel(planes.cpu().numpy(), g["planes"])}
    errs.update({k: common.rel(taps[k].cpu().numpy()[common.TAP_SLICES[k]], g[k]) for k in common.TAPS})
    print(name, errs)
    assert all(e <= common.TOL for e in errs.values()), errs
    assert torch.equal(m(torch.from_numpy(x).to(DEV)), planes)          # a second call, without the taps: bit-identical


def small_reference(seed=73):
    ref = common.Img2PlaneModel("rgb", "small")
    sd = common.weights(seed, "small", 5)
    ref.load_state_dict(dict(sd, **{"low_reso_encoder." + k: v for k, v in ref.low_reso_encoder.state_dict().items()}), strict=True)
    return ref.to(DEV).eval()


def test_from_reference_and_patch_model_give_the_same_planes():
    """from_reference on the plain-torch stand-in of the reference (its state_dict, its own encoder object); patch_model(cano_backbone=True)
    on the mock generator calls the same module; both meet the golden of case b, whose weights these are."""
    from real3dportrait_amd import Img2PlaneModel, patch_model
    g, mode, scale, cin, sd, x = common.golden_case("img2plane_b_s96")
    ref = small_reference()
    xt = torch.from_numpy(x).to(DEV)
    direct = Img2PlaneModel.from_reference(ref)
    assert direct.low_reso_encoder is ref.low_reso_encoder and next(direct.parameters()).is_cuda
    planes = direct(xt)
    assert common.rel(planes.cpu().numpy(), g["planes"]) <= common.TOL
    model = patch_model(mock_model(ref).to(DEV), cano_backbone=True)
    assert type(model.cano_img2plane_backbone) is Img2PlaneModel and model._r3d_reference_cano_backbone is ref
    assert torch.equal(model.cano_img2plane_backbone(xt), planes)
    # the replaced module (eager fp32 torch of the same math) agrees as well
    assert common.rel(model._r3d_reference_cano_backbone(xt).cpu().numpy(), g["planes"]) <= common.TOL


def test_between_feat_low_and_the_planes_everything_is_the_library():
    """From feat_low and the assembled input on: 50 library calls at the small scale (24 + 8 + 18), the attention the new
    kernel, and no torch arithmetic, copy or layout op in between (the planes tensor is allocated, the work buffers are sliced)."""
    import re
    from torch.utils._python_dispatch import TorchDispatchMode
    import abi
    from real3dportrait_amd import _lib
    g, mode, scale, cin, sd, x = common.golden_case("img2plane_b_s96")
    m = common.hip_model(mode, scale, sd, DEV)
    with torch.no_grad():
        x_in = m.assemble_input(torch.from_numpy(x).to(DEV)).contiguous()
        feat_low = m.low_reso_encoder(x_in).contiguous()
        m._run(x_in, feat_low)          # buffers and permuted weights exist from here on

        class Ops(TorchDispatchMode):
            seen = []

            def __torch_dispatch__(self, func, types, args=(), kwargs=None):
                self.seen.append(str(func))
                return func(*args, **(kwargs or {}))
        with _lib.counting() as calls, Ops() as ops:
            planes = m._run(x_in, feat_low)
    names = [c[0] for c in calls]
    assert len(names) == 50 and names.count("r3d_i2p_attention") == 3 and "r3d_secc_attention" not in names
    new = set(abi.header_declarations("r3d_hip_img2plane.h"))
    assert new <= set(names) and set(names) - new == {"r3d_secc_linear", "r3d_secc_conv", "r3d_secc_layernorm", "r3d_secc_dwconv_gelu", "r3d_torso_conv"}
    bad = [o for o in ops.seen if re.search(r"conv|linear|addmm|\bmm\b|bmm|matmul|norm|gelu|relu|softmax|permute|transpose|clone|copy|cat|upsample|shuffle|flip|add|mul",
                                            o)]
    assert not bad, bad
    assert common.rel(planes.cpu().numpy(), g["planes"]) <= common.TOL


def test_on_a_device_that_is_not_the_current_one():
    """Module and image on the last visible GPU while the process's current device stays 0 (with one GPU they are the same device): the
    launches go to the image's device and its current stream.  An image on another device than the parameters is refused."""
    g, mode, scale, cin, sd, x = common.golden_case("img2plane_c_s80_alpha")
    last = "cuda:%d" % (torch.cuda.device_count() - 1)
    m = common.hip_model(mode, scale, sd, last)
    assert torch.cuda.current_device() == 0
    planes = m(torch.from_numpy(x).to(last))
    assert str(planes.device) == last and torch.cuda.current_device() == 0
    assert common.rel(planes.cpu().numpy(), g["planes"]) <= common.TOL
    if last != DEV:
        with pytest.raises(ValueError, match="the module's parameters on"):
            m(torch.from_numpy(x).to(DEV))


def test_a_batch_equals_its_samples_and_weights_are_refolded():
    g, mode, scale, cin, sd, x = common.golden_case("img2plane_c_s80_alpha")
    m = common.hip_model(mode, scale, sd, DEV)
    xt = torch.from_numpy(np.concatenate([x, x[:, :, ::-1].copy()])).to(DEV)
    both = m(xt)
    assert torch.equal(both, m(xt))
    # a sample's planes do not depend on B, given its feat_low: the encoder is torch's (its conv may pick another algorithm for another
    # batch size, and then differs in the last bits), so the samples run alone get the batch's feat_low rows
    with torch.no_grad():
        x_in = m.assemble_input(xt).contiguous()
        feat_low = m.low_reso_encoder(x_in).contiguous()
        assert torch.equal(m._run(x_in, feat_low), both)
        for b in range(2):
            assert torch.equal(both[b:b + 1], m._run(x_in[b:b + 1].contiguous(), feat_low[b:b + 1].contiguous())), b
    assert common.rel(both[:1].cpu().numpy(), g["planes"]) <= common.TOL
    # ref_alphas given: all ones is another input than the rule's mask (the image's first rows are black)
    ones = m(xt[:1].contiguous(), {"ref_alphas": torch.ones(1, 1, 80, 80, device=DEV)})
    assert not torch.equal(ones, both[:1])
    # a parameter modified in place: the permuted conv weights are made again (one staleness rule, _state.py)
    with torch.no_grad():
        m.triplane_predictor_vit.final_conv.weight.mul_(2.0)
        m.triplane_predictor_vit.final_conv.bias.mul_(2.0)
    assert torch.equal(m(xt), both * 2.0)
