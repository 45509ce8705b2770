"""GPU: r3d_torso_seg_input and r3d_torso_mask_volume (include/r3d_hip.h, csrc/r3d_torso_glue.hip) called directly, against
the fp64 restatement of facev2v_warp/model2.py:226-236 (tests/torso_glue_ref64.py).

The parity rule is the kernels' of DESIGN 4.8: e <= max(4 e32, 2^-22) of max|ref|, e32 the error of the reference's own torch calls in
float32 on the CPU against the same restatement.  The exact case needs no rule: with a one-hot segmap resized by 8 every weight is 1/2 and
float32 is exact, so every output equals the fp64 result rounded, bit for bit."""
import numpy as np
import pytest
import torch

import torso_glue_ref64 as G64
from test_torso_forward_host import EXACT, exact_case
from real3dportrait_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64          # floats in front of and behind every output buffer, which the kernels must leave as they are
WORST = {}          # kernel -> (e / bound, e, bound, case): printed by the last test for DESIGN 4.13

# (h, w, Hs, Ws, ksize, D, C, Cs, mul_mask, in_place); N = 2 with two different samples everywhere.
#   4 x 4 with ksize 7: the reflected window covers the whole image;  5 x 7, 12 x 8: no multiple of the 4 x 16 tile;  64 x 64: 64 tiles;
#   segmaps that up-sample (3 x 3), equal the target, down-sample by an integer and by a non-integer ratio;  C 3 and 6 take the
#   one-float path, C 4 and 32 the 16-byte one;  D 1, 3 and 16 give runs of one and of two depth slices a block, D 3 a ragged grid
MASK_CASES = [
    (4, 4, 3, 3, 7, 1, 4, 5, 1, False),
    (4, 4, 4, 4, 7, 16, 32, 6, 1, True),
    (4, 4, 9, 11, 3, 16, 4, 6, 0, False),
    (5, 7, 20, 21, 3, 1, 32, 5, 1, False),
    (5, 7, 13, 9, 1, 16, 4, 6, 0, True),
    (5, 7, 3, 3, 7, 3, 3, 5, 1, False),
    (12, 8, 50, 37, 7, 16, 32, 6, 1, False),
    (12, 8, 3, 3, 3, 1, 4, 5, 1, True),
    (12, 8, 12, 8, 1, 16, 6, 6, 1, True),
    (64, 64, 512, 512, 7, 16, 32, 6, 1, True),
    (64, 64, 100, 77, 3, 1, 4, 5, 0, False),
    (64, 64, 3, 3, 7, 16, 4, 6, 1, False),
    (64, 64, 64, 64, 1, 1, 32, 5, 1, False),
    (64, 64, 128, 192, 7, 1, 32, 6, 0, True),
]
# (Hs, Ws, OH, OW): the same kinds of resize
RESIZE_CASES = [(3, 3, 8, 8), (12, 8, 12, 8), (20, 21, 5, 7), (50, 37, 12, 8), (100, 77, 64, 64), (512, 512, 256, 256), (37, 50, 64, 48)]


def guarded(shape, fill=None):
    """(buffer, view): `view` of `shape` inside a buffer with GUARD patterned floats on each side."""
    n = int(np.prod(shape))
    buf = torch.from_numpy(synth.hash_unitvar(77, (n + 2 * GUARD,))).to(DEV)
    view = buf[GUARD:GUARD + n].view(*shape)
    if fill is not None:
        view.copy_(fill)
    return buf, view


def guards_intact(buf):
    ref = torch.from_numpy(synth.hash_unitvar(77, (buf.numel(),))).to(DEV)
    return torch.equal(buf[:GUARD], ref[:GUARD]) and torch.equal(buf[-GUARD:], ref[-GUARD:])


def note(kernel, e, b, case):
    if kernel not in WORST or e / b > WORST[kernel][0]:
        WORST[kernel] = (e / b, e, b, case)


def run_mask(feats, seg, c0, c1, ksize, mul, in_place):
    """The kernel on NCDHW feats (transposed here): (masked [N, D, h, w, C], motion [N, D, h, w, C + 2]) on the host, guards checked."""
    from real3dportrait_amd import torso_mask_volume
    N, C, D, h, w = feats.shape
    fbuf, f = guarded((N, D, h, w, C), G64.to_cl(torch.from_numpy(feats)).to(DEV))
    before = f.clone()
    mbuf, m = (fbuf, f) if in_place else guarded((N, D, h, w, C))
    obuf, o = guarded((N, D, h, w, C + 2))
    got_m, got_o = torso_mask_volume(f, torch.from_numpy(seg).to(DEV), c0, c1, ksize, mul, masked_cl=m, motion_cl=o)
    torch.cuda.synchronize()
    assert got_m is m and got_o is o
    assert guards_intact(fbuf) and guards_intact(mbuf) and guards_intact(obuf)
    assert in_place or torch.equal(f, before)                               # out of place the input is only read
    return m.cpu(), o.cpu()


@pytest.mark.parametrize("case", MASK_CASES, ids=lambda c: "%dx%d_from_%dx%d_k%d_D%d_C%d_Cs%d_mul%d_%s" % (c[:9] + ("inplace" if c[9] else "out",)))
def test_mask_volume_against_fp64(case):
    h, w, Hs, Ws, ksize, D, C, Cs, mul, in_place = case
    c0, c1 = (2, 4) if Cs == 5 else (5, 1)                                 # Cs 5: the last channel is the reference's 4; Cs 6: its own last
    inp = synth.synth_torso_glue_inputs(300 + h + Hs + ksize, 2, Cs, Hs, Ws, C, D, h, w)
    feats, seg = inp["feats"], inp["segmap"]
    assert not np.array_equal(seg[0], seg[1])
    ref = G64.glue(feats, seg, c0, c1, ksize, bool(mul))
    r32 = G64.torch_glue(feats, seg, c0, c1, ksize, bool(mul))
    masked, motion = run_mask(feats, seg, c0, c1, ksize, mul, in_place)
    for name, got in (("masked", masked), ("motion", motion)):
        want = G64.to_cl(ref[name]).numpy()
        e, e32 = G64.rel(got.numpy(), want), G64.rel(G64.to_cl(r32[name]).numpy(), want)
        print("%s: e %.2e, reference fp32 %.2e, bound %.2e" % (name, e, e32, G64.bound(e32)))
        note("mask_volume", e, G64.bound(e32), case)
        assert e <= G64.bound(e32), (name, e, e32)
    if not mul:
        assert torch.equal(masked, G64.to_cl(torch.from_numpy(feats)))        # a copy
    assert torch.equal(motion[..., :C], masked)                               # the estimator and the generator see the same values
    assert torch.equal(motion[:, 0, :, :, C:], motion[:, D - 1, :, :, C:])     # the pair repeated over depth
    if ksize == 7 and h == 4:                                                  # the window is the whole image: one mask value a sample
        md = ref["mask_d"]
        assert bool((md == md[:, :1, :1]).all()) and float((md[0, 0, 0] - md[1, 0, 0]).abs()) > 1e-3


@pytest.mark.parametrize("name", sorted(EXACT))
def test_mask_volume_exact_case(name):
    """One-hot blobs resized by 8: sum, max and the one multiply are exact, so all outputs equal the fp64 result rounded to fp32."""
    seg, feats, ksize = exact_case(name)
    ref = G64.glue(feats, seg, 2, 4, ksize)
    md = ref["mask_d"].numpy()
    cover = [float((md == 0).mean()), float(((md > 0) & (md < 1)).mean()), float((md == 1).mean())]
    print(name, "mask_d == 0 / between / == 1:", cover)
    assert min(cover) >= 0.05, cover
    for in_place in (False, True):
        masked, motion = run_mask(feats, seg, 2, 4, ksize, 1, in_place)
        assert torch.equal(masked, G64.to_cl(ref["masked"]).float()), in_place
        assert torch.equal(motion, G64.to_cl(ref["motion"]).float()), in_place
    if name == "32x56_to_4x7":                                                # ksize 7 there: the whole image, still exact
        masked, motion = run_mask(feats, seg, 2, 4, 7, 1, False)
        assert torch.equal(motion, G64.to_cl(G64.glue(feats, seg, 2, 4, 7)["motion"]).float())


@pytest.mark.parametrize("Ci", [0, 3])
@pytest.mark.parametrize("case", RESIZE_CASES, ids=lambda c: "%dx%d_to_%dx%d" % c)
def test_seg_input_against_fp64(case, Ci):
    from real3dportrait_amd import torso_seg_input
    Hs, Ws, OH, OW = case
    for Cs, (c0, c1) in ((5, (2, 4)), (6, (5, 0))):
        seg = synth.synth_torso_glue_inputs(400 + Hs + OH, 2, Cs, Hs, Ws, 1, 1, 1, 1)["segmap"]
        img = synth.synth_torso_appearance_inputs(401 + Hs, 2, 3, OH, OW)["x"] if Ci else None
        obuf, out = guarded((2, Ci + 2, OH, OW))
        got = torso_seg_input(None if img is None else torch.from_numpy(img).to(DEV), torch.from_numpy(seg).to(DEV), c0, c1, size=(OH, OW), out=out)
        torch.cuda.synchronize()
        assert got is out and guards_intact(obuf)
        out = out.cpu()
        if Ci:
            assert torch.equal(out[:, :Ci], torch.from_numpy(img))             # the image channels bit for bit
        want = G64.seg_input(None, seg, c0, c1, size=(OH, OW)).numpy()
        e = G64.rel(out[:, Ci:].numpy(), want)
        e32 = G64.rel(G64.torch_seg_input(None, seg, c0, c1, size=(OH, OW)).numpy(), want)
        print("Cs %d: e %.2e, reference fp32 %.2e, bound %.2e" % (Cs, e, e32, G64.bound(e32)))
        note("seg_input", e, G64.bound(e32), case + (Ci, Cs))
        assert e <= G64.bound(e32), (e, e32)
        assert not torch.equal(out[0, Ci:], out[1, Ci:])


def test_seg_input_exact_case():
    from real3dportrait_amd import torso_seg_input
    seg, _, _ = exact_case("512_to_64")
    img = synth.synth_torso_appearance_inputs(5, 2, 3, 256, 256)["x"]          # 512 -> 256: ratio 2, weights 1/2
    out = torso_seg_input(torch.from_numpy(img).to(DEV), torch.from_numpy(seg).to(DEV)).cpu()
    assert torch.equal(out, G64.seg_input(img, seg).float())
    assert {0.0, 0.5, 1.0} <= set(np.unique(out[:, 3:].numpy())) <= {0.0, 0.25, 0.5, 0.75, 1.0}


def test_print_the_worst_cases():
    """Runs last in this file: the worst e / bound per kernel over the cases above (DESIGN 4.13 quotes it)."""
    for k, (frac, e, b, case) in sorted(WORST.items()):
        print("%s: worst e %.2e = %.2f of its bound %.2e at %s" % (k, e, frac, b, case))
        assert frac <= 1.0
