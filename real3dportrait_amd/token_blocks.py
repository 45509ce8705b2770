"""The token-transformer block of the SECC encoder (segformer.py), the image-to-plane ViTs (img2plane.py) and HuBERT (hubert.py), once: the
MiT parameter holders with the reference's attribute names (segformer.py:58-199 of the reference; every state_dict key follows from them), the
channel-last conv weight, and the two launch lists of a block on the r3d_secc_* entry points.

A block works in its model's stream buffers w: "x" the tokens [B, h, wd, C], updated in place; "q", "o", "kv" (and "t", "sr" with spatial
reduction) the attention half's; "h1", "h2" the MLP half's.  `st` is the stream's handle.
"""
import torch.nn as nn

from . import _lib


class PatchEmbed(nn.Module):
    def __init__(self, cin, cout, k, stride):
        super().__init__()
        self.proj = nn.Conv2d(cin, cout, k, stride, k // 2)
        self.norm = nn.LayerNorm(cout)


class Attention(nn.Module):
    def __init__(self, C, sr):
        super().__init__()
        self.q, self.kv, self.proj = nn.Linear(C, C), nn.Linear(C, 2 * C), nn.Linear(C, C)
        self.sr_ratio = sr
        if sr > 1:
            self.sr = nn.Conv2d(C, C, sr, sr)
            self.norm = nn.LayerNorm(C)


class DWConv(nn.Module):
    def __init__(self, hidden):
        super().__init__()
        self.dwconv = nn.Conv2d(hidden, hidden, 3, 1, 1, groups=hidden)


class Mlp(nn.Module):
    def __init__(self, C, hidden):
        super().__init__()
        self.fc1, self.dwconv, self.fc2 = nn.Linear(C, hidden), DWConv(hidden), nn.Linear(hidden, C)


class Block(nn.Module):
    def __init__(self, C, hidden, sr):
        super().__init__()
        self.norm1, self.attn, self.norm2, self.mlp = nn.LayerNorm(C), Attention(C, sr), nn.LayerNorm(C), Mlp(C, hidden)


def conv_weight_cl(w):
    """[Cout, Cin, k, k] -> [Cout, k, k, Cin], what r3d_secc_conv and r3d_torso_conv read."""
    return w.detach().permute(0, 2, 3, 1).contiguous().float()


def attention_half(attention, w, st, B, h, wd, C, heads, n1, q, kv_w, kv_b, proj, sr=1, sr_w=None, sr_b=None, sr_norm=None):
    """x += proj(attention(q(n1(x)), kv(.))): q and kv with n1 as their LayerNorm prologue; with sr > 1 kv reads the sr x sr / stride sr conv
    (weight sr_w channel-last, bias sr_b) of n1(x), under sr_norm as its prologue, so n1(x) is written out once ("t").  `attention` names
    the entry point; n1, q, proj and sr_norm are modules, kv_w / kv_b the (possibly fused) key-value weights.  A sequence is h = T, wd = 1."""
    X, Q, O, KV = w["x"], w["q"], w["o"], w["kv"]
    M, L = B * h * wd, (h // sr) * (wd // sr)
    if sr > 1:
        T, SR = w["t"], w["sr"]
        _lib.call("r3d_secc_layernorm", X, M, C, n1.weight, n1.bias, n1.eps, T, st)
        _lib.call("r3d_secc_linear", T, M, C, None, None, 0.0, q.weight, q.bias, C, 0, None, Q, st)
        _lib.call("r3d_secc_conv", T, B, h, wd, C, sr_w, sr_b, C, sr, sr, 0, None, None, 0.0, SR, st)
        _lib.call("r3d_secc_linear", SR, B * L, C, sr_norm.weight, sr_norm.bias, sr_norm.eps, kv_w, kv_b, 2 * C, 0, None, KV, st)
    else:
        _lib.call("r3d_secc_linear", X, M, C, n1.weight, n1.bias, n1.eps, q.weight, q.bias, C, 0, None, Q, st)
        _lib.call("r3d_secc_linear", X, M, C, n1.weight, n1.bias, n1.eps, kv_w, kv_b, 2 * C, 0, None, KV, st)
    _lib.call(attention, Q, KV, B, h * wd, L, C, heads, (C // heads) ** -0.5, O, st)
    _lib.call("r3d_secc_linear", O, M, C, None, None, 0.0, proj.weight, proj.bias, C, 0, X, X, st)


def mlp_half(w, st, B, h, wd, C, hidden, n2, mlp):
    """x += fc2(gelu(dwconv(fc1(n2(x))))) of a MiT Mlp: n2 as fc1's LayerNorm prologue, the residual in fc2's epilogue."""
    X, H1, H2 = w["x"], w["h1"], w["h2"]
    M, dw = B * h * wd, mlp.dwconv.dwconv
    _lib.call("r3d_secc_linear", X, M, C, n2.weight, n2.bias, n2.eps, mlp.fc1.weight, mlp.fc1.bias, hidden, 0, None, H1, st)
    _lib.call("r3d_secc_dwconv_gelu", H1, B, h, wd, hidden, dw.weight, dw.bias, H2, st)
    _lib.call("r3d_secc_linear", H2, M, hidden, None, None, 0.0, mlp.fc2.weight, mlp.fc2.bias, C, 0, X, X, st)


def mit_block(attention, blk, sr_w, w, st, B, h, wd, C, hidden, heads):
    """One MiT Block (a Block above; sr_w: its attn.sr weight channel-last, or None) on [B, h, wd, C] tokens: seven launches, nine with sr > 1."""
    a = blk.attn
    if a.sr_ratio > 1:
        attention_half(attention, w, st, B, h, wd, C, heads, blk.norm1, a.q, a.kv.weight, a.kv.bias, a.proj, a.sr_ratio, sr_w, a.sr.bias, a.norm)
    else:
        attention_half(attention, w, st, B, h, wd, C, heads, blk.norm1, a.q, a.kv.weight, a.kv.bias, a.proj)
    mlp_half(w, st, B, h, wd, C, hidden, blk.norm2, blk.mlp)
