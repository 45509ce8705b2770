"""Fused HIP evaluation of SuperresolutionHybrid8XDC_Warp.forward, fuse mode 'v2' -- what inference/real3d_infer.py:480-492 runs per
frame with the shipped torso checkpoint (modules/real3d/super_resolution/sr_with_ref.py:67-137; fuse mode from
egs/os_avatar/real3d_orig/secc_img2plane_torso_orig.yaml:29-30).

`patch_model` installs `forward_v2` on the reference's module object (its parameters, its torso_model and its hparams stay where
they are).  Compared with running the reference forward over patched sub-modules:
  * x never takes an NCHW fp32 round trip: block0 -> (alpha blend + concat = input conversion of the next conv) -> fuse_head_torso
    convs -> SynthesisBlockNoUp -> (occlusion blend + concat) -> fuse_fg_bg convs -> block1 hand activations over channel-blocked
    (fp32 at the two blends, fp16 hi/lo SPLIT everywhere else);
  * the resizes, the rgb blends and the occlusion mask are three small HIP kernels (r3d_resize_bilinear / r3d_blend /
    r3d_person_occlusion) instead of ~25 ATen launches;
  * clip constants are computed once: the 512 -> 256 resizes of ref_torso_rgb / ref_bg_rgb and bg_encoder(ref_bg_rgb_256) are cached on
    the identity + version of the input tensors (the reference recomputes them every frame, :79-81,91);
  * fp16 range folding: four r3d_chain_fold launches per frame (block0's; torso_encoder + fuse_head_torso_convs + head_torso_block;
    fuse_fg_bg_convs + block1; block1's conv1 operand), each started from a MEASURED max|x| (taken in a conv epilogue, no extra pass)
    so that no stored operand is more than three layers away from a measurement; a fifth, bg_encoder's, runs once per background image.
The face-vid2vid warp network `torso_model` is a cold-ish PyTorch encoder and is called as is (out of scope).
"""
import torch

from . import _lib
from .sr_activation import _tag, as_input, bound_of, empty, fmt_of, logical_shape, tag_split
from ._state import Derived
from .superresolution import _BoundMeter, _RangeRows, _f32c, blend_cat, chain_fold, const_bound, resize_bilinear

# The two fusions of the v2 forward.  Each has a general form for the shapes it refuses (Conv2d.can_blend, `fuse_cat` below), and
# tests/test_gpu_warp_sr.py::test_warp_sr_forward_v2_round6_fusions_are_bit_identical sets these to False to run that form on the shipped shapes.
_FUSE_BLEND = True           # the person / background blend inside fuse_fg_bg_convs' 1x1 conv (r3d_conv_forward_blend)
_FUSE_TORSO_CAT = True       # torso_encoder writes its half of fuse_head_torso_convs' operand itself (r3d_conv_forward_cat)


def blend(a, b, mask):
    """a * mask + b * (1 - mask)   (sr_with_ref.py:103,113)."""
    a, b, mask = _f32c(a), _f32c(b), _f32c(mask)
    N, C, H, W = a.shape
    assert b.shape == a.shape and tuple(mask.shape) == (N, 1, H, W)
    out = torch.empty_like(a)
    _lib.call("r3d_blend", a, b, mask, N, C, H, W, out)
    return out


def person_occlusion(alpha, torso_occlusion, head_threshold):
    """clamp(torso_occlusion + where(alpha > thr, 1, alpha), 0, 1)   (sr_with_ref.py:117-122)."""
    alpha, torso_occlusion = _f32c(alpha), _f32c(torso_occlusion)
    assert alpha.shape == torso_occlusion.shape
    out = torch.empty_like(alpha)
    _lib.call("r3d_person_occlusion", alpha, torso_occlusion, float(head_threshold), alpha.numel(), out)
    return out


def _measured(t):
    """Tag a (clip-constant) fp32 activation with its MEASURED max|x| (its own tensor, not a meter row that later calls reuse)."""
    return _tag(t, _BoundMeter()(t).clone(), 0)


class WarpSRState:
    """Per-module scratch of the fused forward (range rows, meters, clip-constant caches)."""

    def __init__(self, hparams):
        self.hparams = dict(hparams)
        self.rows = _RangeRows(3)           # max|x0| (block0), max|x2| (head_torso_block), max|z| (fuse_fg_bg_convs): measured in the epilogues
        self.split_fold_pending = False     # split_input_spec() folded block0 for a SPLIT input that forward() has not consumed yet
        self.meter_x, self.meter_hid = _BoundMeter(), _BoundMeter()
        self.c_torso256, self.c_bg256, self.c_xbg, self.c_ws3 = Derived(), Derived(), Derived(), Derived()


def warp_split_input_spec(self, ws, N, dev):
    """As SuperresolutionHybrid8XDC.split_input_spec, for the fused Warp forward: block0's styles and range fold for the renderer's
    feature image (|x| <= 1.01) are put in place NOW (the fold also clears the max|x0| row block0's epilogue measures into), and
    (folded input multiplier, per-sample stride in floats, consuming block) is returned for r3d_render_forward's split_out.  The
    caller hands the SPLIT tensor to the next forward() as `x`; None when the precision has no SPLIT operand."""
    S = self._r3d_state
    b0 = self.block0
    if b0.precision not in ("f16x3", "f16mx") or self.input_resolution != 128:
        return None
    ws3 = S.c_ws3.get([ws], lambda: ws[:, -1:, :].expand(N, 3, -1).contiguous())
    b0.prepare(ws3, dev, ws_key=ws)
    chain_fold([b0.chain_op(-1)], N, [const_bound(1.01, N, dev)], zero=[S.rows.at(N, dev)[0]])
    S.split_fold_pending = True
    scale, stride = b0.in_scale()
    return scale, stride, b0


def forward_v2(self, rgb, x, ws, ref_torso_rgb, ref_bg_rgb, weights_img, segmap, kp_s, kp_d, target_torso_mask=None, **block_kwargs):
    """Signature and return value of SuperresolutionHybrid8XDC_Warp.forward (sr_with_ref.py:67): (rgb [N,3,512,512], facev2v_ret)."""
    S = self._r3d_state
    hp = S.hparams
    if hp.get("weight_fuse", True) and hp.get("htbsr_head_weight_fuse_mode") == "v1" and getattr(self, "_r3d_reference_forward", None) is None:
        # fuse mode v1 (sr_with_ref.py:92-104; not the shipped configuration): the direct alpha blend of x and x_torso -- the flow of the two-stage
        # entry with the hparams' head threshold.  Operator by operator (each folds its own range), not fused.
        return _forward_v1(self, rgb, x, ws, ref_torso_rgb, ref_bg_rgb, weights_img, segmap, kp_s, kp_d, target_torso_mask, block_kwargs)
    if not hp.get("weight_fuse", True) or hp.get("htbsr_head_weight_fuse_mode") != "v2":
        ref_forward = getattr(self, "_r3d_reference_forward", None)
        if ref_forward is not None:        # a patch_model()'d reference module: its own forward over the patched sub-modules
            return ref_forward(rgb, x, ws, ref_torso_rgb, ref_bg_rgb, weights_img, segmap, kp_s, kp_d, target_torso_mask=target_torso_mask, **block_kwargs)
        raise NotImplementedError("the HIP forward covers weight_fuse=True with htbsr_head_weight_fuse_mode 'v2' (fused: the shipped torso model) and 'v1' "
                                  "(operator by operator); 'v3' adds a learned mask post-processing (head_torso_alpha_predictor) that is not built")
    if self.block0.precision == "f32":
        # the exact-f32 kernels have no channel-blocked hand-off / epilogue measurements: run the reference's own forward over the
        # patched sub-modules (patch_model keeps it), or refuse for the mirror class that has none
        ref_forward = getattr(self, "_r3d_reference_forward", None)
        if ref_forward is None:
            raise NotImplementedError("the fused SuperresolutionHybrid8XDC_Warp forward needs SR precision 'f16x3' (got 'f32')")
        return ref_forward(rgb, x, ws, ref_torso_rgb, ref_bg_rgb, weights_img, segmap, kp_s, kp_d, target_torso_mask=target_torso_mask,
                           **block_kwargs)
    return _forward_v2(self, S, rgb, x, ws, ref_torso_rgb, ref_bg_rgb, weights_img, segmap, kp_s, kp_d, target_torso_mask, block_kwargs)


def _prologue(self, rgb, x, ws, ref_torso_rgb, ref_bg_rgb, weights_img, block_kwargs, cache=None):
    """What every entry point does before block0 (sr_with_ref.py:69-82, :167-178): ws3, the resize to input_resolution where x has another,
    the four 256^2 resizes, noise_mode 'none' unless the caller names one.  cache: the WarpSRState whose entries keep what is constant over
    a clip (ws3, the two reference resizes) -- the fused forward's; None: computed on every call.
    Returns (x, rgb, ws3, rgb_256, weights_256, ref_torso_rgb_256, ref_bg_rgb_256, block keywords)."""
    aa, N = self.sr_antialias, rgb.shape[0]
    once = lambda name, src, fn: fn() if cache is None else getattr(cache, name).get([src], fn)
    to256 = lambda t: resize_bilinear(t, (256, 256), aa)
    ws3 = once("c_ws3", ws, lambda: ws[:, -1:, :].expand(N, 3, -1).contiguous())                        # :69
    if fmt_of(x) != "split" and x.shape[-1] != self.input_resolution:                                   # :71-75, cold
        sz = (self.input_resolution, self.input_resolution)
        x, rgb = resize_bilinear(x, sz, aa), resize_bilinear(rgb, sz, aa)
    rgb_256 = to256(rgb)                                                                                # :77
    weights_256 = to256(weights_img.detach())                                                           # :78
    ref_torso_rgb_256 = once("c_torso256", ref_torso_rgb, lambda: to256(ref_torso_rgb))                 # :80 (clip constant)
    ref_bg_rgb_256 = once("c_bg256", ref_bg_rgb, lambda: to256(ref_bg_rgb))                             # :82 (clip constant)
    kw = dict(block_kwargs)
    kw.setdefault("noise_mode", "none")
    return x, rgb, ws3, rgb_256, weights_256, ref_torso_rgb_256, ref_bg_rgb_256, kw


def _torso_forward(self, ref_torso_rgb_256, segmap, kp_s, kp_d, rgb_256, weights_256, target_torso_mask):
    """The warp-based torso branch (PyTorch, untouched) (:84-87): a v2 torso model also takes the head weights."""
    v1 = self._r3d_state.hparams.get("torso_model_version", "v1") == "v1"
    return self.torso_model.forward(ref_torso_rgb_256, segmap, kp_s, kp_d, rgb_256.detach(), *(() if v1 else (weights_256.detach(),)),
                                    cal_loss=True, target_torso_mask=target_torso_mask)


def _forward_v1(self, rgb, x, ws, ref_torso_rgb, ref_bg_rgb, weights_img, segmap, kp_s, kp_d, target_torso_mask, block_kwargs):
    hp, aa = self._r3d_state.hparams, self.sr_antialias
    x, rgb, ws3, rgb_256, weights_256, ref_torso_rgb_256, ref_bg_rgb_256, kw = _prologue(self, rgb, x, ws, ref_torso_rgb, ref_bg_rgb, weights_img, block_kwargs)
    kw.update(_out_format="nchw", _return_x=True)         # the blocks are shared with the fused forward: the reference layout for these calls only
    x, rgb = self.block0(x, rgb, ws3, **kw)                                                             # :83
    rgb_torso, ret = _torso_forward(self, ref_torso_rgb_256, segmap, kp_s, kp_d, rgb_256, weights_256, target_torso_mask)
    x_torso = self.torso_encoder(ret["deformed_torso_hid"])                                             # :88
    x_bg = self.bg_encoder(ref_bg_rgb_256)                                                              # :90
    rgb = blend(rgb, rgb_torso, weights_256)                                                            # :94
    x = blend(x, x_torso, weights_256)                                                                  # :95
    torso_occ = resize_bilinear(ret["occlusion_2"], (256, 256), aa)                                     # :99
    pocc = person_occlusion(weights_256, torso_occ, hp["htbsr_head_threshold"])                         # :96-100
    rgb = blend(rgb, ref_bg_rgb_256, pocc)                                                              # :101
    x = self.fuse_fg_bg_convs(blend_cat(x, x_bg, pocc, self.fuse_fg_bg_convs))                          # :102-103
    _, rgb = self.block1(x, rgb, ws3, **kw)                                                             # :104
    return rgb, ret


def _forward_v2(self, S, rgb, x, ws, ref_torso_rgb, ref_bg_rgb, weights_img, segmap, kp_s, kp_d, target_torso_mask, block_kwargs):
    hp, aa = S.hparams, self.sr_antialias
    N, dev = rgb.shape[0], rgb.device
    x, rgb, ws3, rgb_256, weights_256, ref_torso_rgb_256, ref_bg_rgb_256, kw = _prologue(self, rgb, x, ws, ref_torso_rgb, ref_bg_rgb, weights_img, block_kwargs, cache=S)
    b0, b1, hb = self.block0, self.block1, self.head_torso_block
    fuse_ht, fuse_fg = self.fuse_head_torso_convs, self.fuse_fg_bg_convs
    m_x0, m_x2, m_z = S.rows.at(N, dev)

    # ---- block0: 128^2 head features -> 256^2 (:83); its conv1 epilogue measures max|x0| ------------------------------------------
    prep0 = b0.prepare(ws3, dev, ws_key=ws)
    x, _, presplit = as_input(x, b0)
    if presplit and not S.split_fold_pending:
        # (the ray kernel wrote block0's first operand itself: split_input_spec above folded for it before the render launch)
        raise RuntimeError("SPLIT feature image without a pending split_input_spec() fold of this module")
    S.split_fold_pending = False
    if not presplit:
        bx, _ = bound_of(x, S.meter_x, layers=2)
        chain_fold([b0.chain_op(-1)], N, [bx], zero=[m_x0])
    # block0 / head_torso_block / block1 are shared with the reference's other entry points (infer_forward_stage1/2, sr_with_ref.py:165-214, call
    # self.block0(x, rgb, ws) and expect NCHW x): the hand-off formats are per call
    x0, rgb0 = b0(x, rgb, ws3, _prepared=prep0, _folded=True, _x_absmax=m_x0, _out_format="cb8", _return_x=True, **kw)

    rgb_torso, ret = _torso_forward(self, ref_torso_rgb_256, segmap, kp_s, kp_d, rgb_256, weights_256, target_torso_mask)          # :84-87
    hid = ret["deformed_torso_hid"]
    te = self.torso_encoder._plan() if _FUSE_TORSO_CAT else ()
    _, Ca, H0, W0 = logical_shape(x0)
    fuse_cat = len(te) == 1 and te[0][0].kernel_size[0] == 1 and te[0][0].out_channels % 16 == 0 and fmt_of(x0) == "cb8" \
        and Ca % 16 == 0 and fmt_of(hid) == "nchw"
    if not fuse_cat:
        x_torso = self.torso_encoder(hid, out_format="cb8")                                            # :88 (1x1 conv, measured input)
    x_bg = S.c_xbg.get([ref_bg_rgb], lambda: _measured(self.bg_encoder(ref_bg_rgb_256, out_format="cb8")))   # :90 (clip constant)

    # ---- head / torso fusion (:99-105) -----------------------------------------------------------------------------------------------
    alpha = weights_256                                   # `head_torso_alpha[head_torso_alpha > weights_256] = ...` (:101-102) is a no-op
    rgb1 = blend(rgb0, rgb_torso, alpha)                                                                # :103
    preph = hb.prepare(ws3, dev, ws_key=ws)
    if fuse_cat:
        # torso_encoder writes its half of :104's concatenation itself (r3d_conv_forward_cat): x_torso * (1 - alpha), times fuse_head_torso_convs' in-multiplier,
        # split -- the fp32 x_torso (67 MB written, 67 MB read back by blend_cat) does not exist.  The consumer's fold therefore runs BEFORE the producer, in one
        # chain with it: op 0 = torso_encoder (bound of its output = what its tag carried), op 1.. = the fusion stack reading (max|x0|, op 0).  Same bits.
        tconv, tslope, _ = te[0]
        hid, _, _ = as_input(hid, tconv)
        tconv.prepare(N, dev)
        bh, dh = bound_of(hid, S.meter_hid, 1)
        tconv._depth_in = dh
        ops, head, last = fuse_ht.chain_ops(N, dev, -2, 0, base=1)
        chain_fold([tconv.chain_op(-1, negative_slope=tslope)] + ops + [hb.chain_op(last)], N, [bh, m_x0], zero=[m_x2])
        fmt = "split_mx" if head.wants_mx() else "split"
        Cb = tconv.out_channels
        xs = tag_split(empty(fmt, N, Ca + Cb, H0, W0, dev), fmt, head)
        tconv.forward_cat(hid, xs, Ca, alpha, True, head, negative_slope=tslope)
        blend_cat(x0, None, alpha, fuse_ht, _folded_head=head, _b_channels=Cb, _dst=xs)
    else:
        ops, head, last = fuse_ht.chain_ops(N, dev, -1, -2, base=0)
        chain_fold(ops + [hb.chain_op(last)], N, [m_x0, bound_of(x_torso, S.meter_hid, 3)[0]], zero=[m_x2])
        xs = blend_cat(x0, x_torso, alpha, fuse_ht, _folded_head=head)                                  # :104
    # head_torso_block's conv1 operand is three layers from the measured max|x0| (= MAX_DEPTH): the fold above covers it, and cleared the
    # row the block measures max|x2| into
    y = fuse_ht(xs, out_format="split_mx" if hb.wants_mx() else "split", _next=hb)                     # :105
    x2, rgb2 = hb(y, rgb1, ws3, _prepared=preph, _folded=True, _x_absmax=m_x2, _out_format="cb8", _return_x=True, **kw)      # :106

    # ---- person / background fusion (:107-115) ----------------------------------------------------------------------------------------
    torso_occ = resize_bilinear(ret["occlusion_2"], (256, 256), aa)                                     # :110
    pocc = person_occlusion(alpha, torso_occ, hp["htbsr_head_threshold"])                              # :107-111
    rgb3 = blend(rgb2, ref_bg_rgb_256, pocc)                                                            # :112
    prep1 = b1.prepare(ws3, dev, ws_key=ws)
    ops, head, last = fuse_fg.chain_ops(N, dev, -1, -2, base=0)
    chain_fold(ops + [b1.chain_op(last)], N, [m_x2, x_bg._r3d_bound], zero=[m_z])
    # f16mx: the last fusion conv leaves fp8 records for block1's up-sampling conv (R3D_FMT_SPLIT_MX), as block0 does in the head-only network
    zfmt = "split_mx" if b1.wants_mx() else "split"
    if _FUSE_BLEND and head.can_blend(x2, x_bg):
        # :113 inside the 1x1 conv of :114 (r3d_conv_forward_blend): the 512-channel concatenation is never written (bit-identical to the two-step form)
        z = fuse_fg(None, out_format=zfmt, _next=b1, _y_absmax=m_z, _blend=(x2, x_bg, pocc))
    else:
        xs2 = blend_cat(x2, x_bg, pocc, fuse_fg, _folded_head=head)                                     # :113
        z = fuse_fg(xs2, out_format=zfmt, _next=b1, _y_absmax=m_z)                                      # :114
    chain_fold([b1.chain_op(-1, tail=True)], N, [m_z])
    _, rgb_out = b1(z, rgb3, ws3, _prepared=prep1, _folded=True, _return_x=False, **kw)                # :115
    return rgb_out, ret


@torch.no_grad()
def infer_forward_stage1(self, rgb, x, ws, ref_torso_rgb, ref_bg_rgb, weights_img, segmap, kp_s, kp_d, **block_kwargs):
    """sr_with_ref.py:164-188 (the reference's two-stage entry, unused by real3d_infer.py): block0 + the warp network's first stage; returns
    the dict the second stage continues from (keys as the reference: the torso model's own + 'ref_bg_rgb_256', 'weights_256', 'x', 'ws',
    'rgb').  Runs the HIP operators one by one (each folds its own range): the fused per-frame path is `forward`."""
    x, rgb, ws3, rgb_256, weights_256, ref_torso_rgb_256, ref_bg_rgb_256, kw = _prologue(self, rgb, x, ws, ref_torso_rgb, ref_bg_rgb, weights_img, block_kwargs)  # :167-178
    x, rgb = self.block0(x, rgb, ws3, _out_format="nchw", _return_x=True, **kw)                         # :180
    ret = self.torso_model.infer_forward_stage1(ref_torso_rgb_256, segmap, kp_s, kp_d, rgb_256.detach(), cal_loss=True)      # :182
    ret["ref_bg_rgb_256"], ret["weights_256"], ret["x"], ret["ws"], ret["rgb"] = ref_bg_rgb_256, weights_256, x, ws3, rgb
    return ret


@torch.no_grad()
def infer_forward_stage2(self, facev2v_ret, **block_kwargs):
    """sr_with_ref.py:190-218: the warp network's second stage, the alpha / occlusion blends, fuse_fg_bg_convs, block1 -> (rgb, ret).
    (This entry blends x and x_torso directly -- no fuse_head_torso_convs / head_torso_block -- and thresholds the head mask at 0.5.)"""
    hp = self._r3d_state.hparams
    x, ws3, rgb = facev2v_ret["x"], facev2v_ret["ws"], facev2v_ret["rgb"]
    ref_bg_rgb_256, weights_256 = facev2v_ret["ref_bg_rgb_256"], facev2v_ret["weights_256"]
    rgb_torso = self.torso_model.infer_forward_stage2(facev2v_ret)                                      # :196
    x_torso = self.torso_encoder(facev2v_ret["deformed_torso_hid"])                                     # :197
    x_bg = self.bg_encoder(ref_bg_rgb_256)                                                              # :198
    kw = dict(block_kwargs)
    kw.setdefault("noise_mode", "none")
    if not hp.get("weight_fuse", True):
        raise NotImplementedError("weight_fuse=False: block1 is called with img=None there (sr_with_ref.py:214-216), which the HIP "
                                  "SynthesisBlock does not build")
    rgb = blend(rgb, rgb_torso, weights_256)                                                            # :201
    x = blend(x, x_torso, weights_256)                                                                  # :202
    torso_occ = resize_bilinear(facev2v_ret["occlusion_2"], (256, 256), self.sr_antialias)             # :206
    pocc = person_occlusion(weights_256, torso_occ, 0.5)                                                # :204-207
    rgb = blend(rgb, ref_bg_rgb_256, pocc)                                                              # :209
    x = self.fuse_fg_bg_convs(blend_cat(x, x_bg, pocc, self.fuse_fg_bg_convs))                          # :210-211
    x, rgb = self.block1(x, rgb, ws3, _out_format="nchw", _return_x=True, **kw)                         # :212
    return rgb, facev2v_ret


class SuperresolutionHybrid8XDC_Warp(torch.nn.Module):
    """Mirror of the reference class (sr_with_ref.py:16-63) for weight_fuse=True with fuse mode 'v2' (the shipped configuration; fused forward) or 'v1'
    (operator by operator; like the reference it then has no head_torso_alpha_predictor / fuse_head_torso_convs / head_torso_block): same
    attribute names and state_dict keys for everything except `torso_model`, which is PASSED IN (the reference's face-vid2vid
    network, any module with its forward signature); forward = the fused HIP evaluation above.  `patch_model` does not need this
    class (it converts a constructed reference module in place); it serves callers that build the pipeline without the reference."""

    def __init__(self, channels, img_resolution, sr_num_fp16_res, sr_antialias, torso_model=None, hparams=None, **block_kwargs):
        super().__init__()
        from .superresolution import Conv2d, ConvStack, SynthesisBlock, SynthesisBlockNoUp
        nn = torch.nn
        assert img_resolution == 512 and sr_num_fp16_res == 0
        hp = {"weight_fuse": True, "htbsr_head_weight_fuse_mode": "v2", "htbsr_head_threshold": 0.9, "torso_model_version": "v2"}
        hp.update(hparams or {})
        self.input_resolution, self.sr_antialias = 128, sr_antialias
        self.block0 = SynthesisBlock(channels, 256, w_dim=512, resolution=256, img_channels=3, is_last=False, use_fp16=False,
                                     conv_clamp=None, **block_kwargs)
        self.block1 = SynthesisBlock(256, 128, w_dim=512, resolution=512, img_channels=3, is_last=True, use_fp16=False,
                                     conv_clamp=None, **block_kwargs)
        self.torso_model = torso_model
        lrelu = nn.LeakyReLU
        self.torso_encoder = ConvStack(Conv2d(64, 256, 1, 1, padding=0))
        self.bg_encoder = ConvStack(Conv2d(3, 64, 3, 1, padding=1), lrelu(), Conv2d(64, 256, 3, 1, padding=1), lrelu(),
                                    Conv2d(256, 256, 3, 1, padding=1))
        if hp.get("weight_fuse", True) and hp.get("htbsr_head_weight_fuse_mode") != "v1":
            # the reference builds these three for every fuse mode except v1 (sr_with_ref.py:36-54): a v1 checkpoint has no such keys and must load strict=True.
            # head_torso_alpha_predictor is unused by fuse mode v2 and stays plain torch.
            self.head_torso_alpha_predictor = nn.Sequential(nn.Conv2d(3 + 1 + 3, 32, 3, 1, padding=1), lrelu(), nn.Conv2d(32, 32, 3, 1, padding=1),
                                                            lrelu(), nn.Conv2d(32, 1, 3, 1, padding=1), nn.Sigmoid())
            self.fuse_head_torso_convs = ConvStack(Conv2d(512, 256, 3, 1, padding=1), lrelu(), Conv2d(256, 256, 3, 1, padding=1))
            self.head_torso_block = SynthesisBlockNoUp(256, 256, w_dim=512, resolution=256, img_channels=3, is_last=False, use_fp16=False,
                                                       conv_clamp=None, **block_kwargs)
        self.fuse_fg_bg_convs = ConvStack(Conv2d(512, 64, 1, 1, padding=0), lrelu(), Conv2d(64, 256, 3, 1, padding=1), lrelu(),
                                          Conv2d(256, 256, 3, 1, padding=1))
        self._r3d_state = WarpSRState(hp)

    forward = forward_v2
    infer_forward_stage1 = infer_forward_stage1
    infer_forward_stage2 = infer_forward_stage2

    def split_input_spec(self, ws, N, dev):
        return warp_split_input_spec(self, ws, N, dev)
