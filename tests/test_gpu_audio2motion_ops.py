"""GPU: the three entry points of include/r3d_hip_audio.h against fp64 at their edges, each within 2e-4 of max|ref| (the project's
tolerance) and bit-identical on a second run.  Shapes are the smallest at which a path can go wrong: one row, rows and channels that
are no multiple of a tile, more than one block in every grid dimension, the WN tile R3D_A2M_WN_ROWS minus one, exactly, plus one."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import audio2motion_ref64 as ref64
from real3dportrait_amd import synth
from real3dportrait_amd import audio2motion as a2m

pytestmark = pytest.mark.gpu
TOL = 2e-4
R = a2m.WN_ROWS
DEV = "cuda:0"


def rnd(seed, *shape, scale=1.0):
    return torch.from_numpy(synth.hash_unitvar(seed, shape) * np.float32(scale))


def close(got, ref, what):
    ref = ref.double()
    err = float((got.double().cpu() - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)
    print("%s: %.2e of max|ref|" % (what, err))
    assert err <= TOL, (what, err)


# ---- conv1d ------------------------------------------------------------------------------------------------------------------------------
def conv1d_ref(c, t):
    """fp64 restatement of r3d_a2m_conv1d on CPU tensors; returns the whole y buffer (columns outside the slice keep their fill)."""
    B, Tin, Cin, Cout, k = c["B"], c["T"], c["Cin"], c["Cout"], c["k"]
    d = lambda v: None if v is None else v.double()
    x = t["x"].double()[:, :, c["xo"]:c["xo"] + Cin]
    if c["mode"] == 1:
        x = x[:, 0::2]
    elif c["mode"] == 2:
        x = 0.5 * (x[:, 0::2] + x[:, 1::2])
    r = F.conv1d(x.transpose(1, 2), t["w"].double().permute(0, 2, 1), d(t.get("bias")), stride=c["stride"], padding=c["pad"]).transpose(1, 2)
    Tout = r.shape[1]
    if "table" in t:
        r = r + t["table"].double()[t["idx"][:, ::c["step"]]]
    for n in ("0", "1"):
        if "amp" + n in t:
            r = r + t["amp" + n].double()[:, None, None] * t["u" + n].double()
    if c["gelu"]:
        r = F.gelu(r)
    if "mask" in t:
        r = r * t["mask"].double().unsqueeze(-1)
    y = t["y0"].double().clone()
    cols = torch.arange(c["yo"], c["yo"] + Cout)
    if c["flip"]:
        cols = c["ys"] - 1 - cols
    if c["sub"]:
        r = y[:, :, cols] - r
    y[:, :, cols] = r
    return y, Tout


def conv_case(seed, B=1, T=7, Cin=5, Cout=6, k=3, stride=1, pad=None, mode=0, xs=None, xo=0, ys=None, yo=0, flip=0, gelu=0, sub=0, bias=1,
              mask=0, table=0, step=1, amps=0):
    pad = k // 2 if pad is None else pad
    c = dict(B=B, T=T, Cin=Cin, Cout=Cout, k=k, stride=stride, pad=pad, mode=mode, xs=xs or Cin, xo=xo, ys=ys or Cout, yo=yo, flip=flip, gelu=gelu,
             sub=sub, step=step)
    Tout = (T + 2 * pad - k) // stride + 1
    t = {"x": rnd(seed, B, T * (2 if mode else 1), c["xs"]), "w": rnd(seed + 1, Cout, k, Cin, scale=(k * Cin) ** -0.5), "y0": rnd(seed + 2, B, Tout, c["ys"])}
    if bias:
        t["bias"] = rnd(seed + 3, Cout, scale=0.3)
    if mask:
        t["mask"] = (torch.from_numpy(synth.hash_uniform(seed + 4, B * Tout)).reshape(B, Tout) > 0.4).float() * 1.5
    if table:
        t["table"] = rnd(seed + 5, 3, Cout)
        t["idx"] = (torch.from_numpy(synth.hash_uniform(seed + 6, B * Tout * step)).reshape(B, Tout * step) * 3).long()
    for n in range(amps):
        t["amp%d" % n], t["u%d" % n] = rnd(seed + 7 + n, B), rnd(seed + 9 + n, Cout)
    return c, t


CONV_CASES = {}
for _T in (1, 2, 7):
    for _k in (1, 3, 8):
        for _mode in (0, 1, 2):
            CONV_CASES["T%d_k%d_mode%d" % (_T, _k, _mode)] = dict(T=_T, k=_k, mode=_mode, B=2)
CONV_CASES.update({
    "no_bias": dict(bias=0), "gelu": dict(gelu=1), "mask": dict(mask=1, B=2), "table": dict(table=1, B=2), "table_step2": dict(table=1, step=2, B=2),
    "amp": dict(amps=1, B=2), "amp2": dict(amps=2, B=2), "subtract": dict(sub=1), "flip": dict(flip=1, ys=16, yo=8, Cout=8),
    "slice_in": dict(xs=11, xo=4), "slice_out": dict(ys=13, yo=5),
    "all_pieces": dict(B=2, T=7, k=3, mode=1, gelu=1, mask=1, table=1, step=2, amps=2, sub=1, flip=1, xs=9, xo=3, ys=14, yo=2),
    "coupling_post": dict(B=2, T=5, Cin=64, Cout=8, k=1, sub=1, flip=1, ys=16, yo=8),
    "g_pre_net": dict(B=2, T=20, Cin=12, Cout=12, k=8, stride=4, pad=2),
    "stride3_ragged": dict(T=11, k=5, stride=3, pad=1),
    "many_blocks": dict(B=2, T=70, Cin=37, Cout=45, k=3, mode=2, gelu=1, mask=1),          # 3 row tiles x 2 column tiles x 2 samples, K = 111
    "transposed_conv_view": dict(B=2, T=3, Cin=16, Cout=4 * 40, k=1),
})


@pytest.mark.parametrize("name", list(CONV_CASES))
def test_conv1d(name):
    c, t = conv_case(100 + 17 * list(CONV_CASES).index(name), **CONV_CASES[name])
    ref, Tout = conv1d_ref(c, t)
    g = {k: v.to(DEV) for k, v in t.items()}

    def run():
        y = g["y0"].clone()
        a2m.conv1d(g["x"], c["B"], c["T"], c["Cin"], g["w"], y, k=c["k"], stride=c["stride"], pad=c["pad"], bias=g.get("bias"), x_stride=c["xs"],
                   x_offset=c["xo"], row_mode=c["mode"], gelu=c["gelu"], mask=g.get("mask"), table=g.get("table"), idx=g.get("idx"), idx_step=c["step"],
                   amp0=g.get("amp0"), u0=g.get("u0"), amp1=g.get("amp1"), u1=g.get("u1"), subtract_from=y if c["sub"] else None,
                   y_stride=c["ys"], y_offset=c["yo"], flip_out=c["flip"])
        return y
    x_before = g["x"].clone()
    y = run()
    close(y, ref, "conv1d " + name)
    cols = torch.ones(c["ys"], dtype=torch.bool)
    lo = c["ys"] - c["yo"] - c["Cout"] if c["flip"] else c["yo"]
    cols[lo:lo + c["Cout"]] = False
    assert torch.equal(y[:, :, cols].cpu(), t["y0"][:, :, cols]), "columns outside the slice were written"
    assert torch.equal(g["x"], x_before) and torch.equal(run(), y)


def test_conv1d_subtract_from_another_buffer():
    c, t = conv_case(900, B=2, T=6, Cin=9, Cout=8, ys=16, yo=8, sub=1)
    ref, _ = conv1d_ref(c, t)
    g = {k: v.to(DEV) for k, v in t.items()}
    y = torch.full_like(g["y0"], 7.0)
    a2m.conv1d(g["x"], 2, 6, 9, g["w"], y, k=3, pad=1, bias=g["bias"], subtract_from=g["y0"], y_stride=16, y_offset=8)
    close(y[:, :, 8:], ref[:, :, 8:], "conv1d subtract_from another buffer")
    assert bool((y[:, :, :8] == 7.0).all())


# ---- wn_layer ----------------------------------------------------------------------------------------------------------------------------
def wn_ref(x, g, w_in, b_in, w_rs, b_rs, mask, out0, k, first, last):
    x, g, H, T = x.double(), g.double(), x.shape[2], x.shape[1]
    xp = F.pad(x, (0, 0, k // 2, k // 2))
    a = torch.cat([xp[:, j:j + T] for j in range(k)] + [g], -1) @ w_in.double() + b_in.double()
    rs = (torch.tanh(a[..., :H]) * torch.sigmoid(a[..., H:])) @ w_rs.double() + b_rs.double()
    m = mask.double().unsqueeze(-1)
    if last:
        return None, ((rs if first else out0.double() + rs) * m)
    return (x + rs[..., :H]) * m, (rs[..., H:] if first else out0.double() + rs[..., H:])


@pytest.mark.parametrize("pos", ["first", "middle", "last"])
@pytest.mark.parametrize("T", [1, R - 1, R, R + 1])
@pytest.mark.parametrize("H,k,Cg", [(64, 3, 128), (256, 5, 64)])
def test_wn_layer(H, k, Cg, T, pos):
    B, seed = 2, 1000 + H + 7 * T + {"first": 0, "middle": 1, "last": 2}[pos]
    first, last = pos == "first", pos == "last"
    K, Crs = k * H + Cg, H if last else 2 * H
    t = {"x": rnd(seed, B, T, H), "g": rnd(seed + 1, B, T, Cg), "w_in": rnd(seed + 2, K, 2 * H, scale=1.5 * K ** -0.5), "b_in": rnd(seed + 3, 2 * H, scale=0.3),
         "w_rs": rnd(seed + 4, H, Crs, scale=2.0 * H ** -0.5), "b_rs": rnd(seed + 5, Crs, scale=0.3), "out0": rnd(seed + 6, B, T, H)}
    t["mask"] = torch.ones(B, T)
    t["mask"][1, T // 2:] = 0.0
    xn_ref, out_ref = wn_ref(t["x"], t["g"], t["w_in"], t["b_in"], t["w_rs"], t["b_rs"], t["mask"], t["out0"], k, first, last)
    g = {n: v.to(DEV) for n, v in t.items()}
    layer = {n: g[n] for n in ("w_in", "b_in", "w_rs", "b_rs")}

    def run():
        out, xn = g["out0"].clone(), None if last else torch.full_like(g["x"], float("nan"))
        a2m.wn_layer(g["x"], g["g"], B, T, H, Cg, k, layer, g["mask"], first, last, xn, out)
        return xn, out
    xn, out = run()
    what = "wn_layer H%d k%d T%d %s" % (H, k, T, pos)
    close(out, out_ref, what + " out")
    if not last:
        close(xn, xn_ref, what + " x_next")
    assert torch.equal(g["x"].cpu(), t["x"]) and torch.equal(g["g"].cpu(), t["g"]), "an input buffer was written"
    xn2, out2 = run()
    assert torch.equal(out2, out) and (last or torch.equal(xn2, xn))


def test_wn_layer_without_mask_is_mask_of_ones():
    B, T, H, Cg, k = 1, R + 3, 64, 128, 3
    K = k * H + Cg
    g = {"x": rnd(1, B, T, H), "g": rnd(2, B, T, Cg), "w_in": rnd(3, K, 2 * H, scale=K ** -0.5), "b_in": rnd(4, 2 * H), "w_rs": rnd(5, H, 2 * H, scale=H ** -0.5),
         "b_rs": rnd(6, 2 * H)}
    g = {n: v.to(DEV) for n, v in g.items()}
    outs = []
    for mask in (None, torch.ones(B, T, device=DEV)):
        out, xn = torch.empty(B, T, H, device=DEV), torch.empty(B, T, H, device=DEV)
        a2m.wn_layer(g["x"], g["g"], B, T, H, Cg, k, g, mask, True, False, xn, out)
        outs.append((out, xn))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


# ---- pitch_embed -------------------------------------------------------------------------------------------------------------------------
def test_pitch_embed_indices_are_the_fp64_ones():
    B, T, C = 2, 2 * R + 4, 24
    f0 = synth.synth_audio2motion_inputs(31, B, T)["f0"]                  # every value at least 2e-3 from an index edge
    f0[0, 0:12:2] = [0.0, 30.0, 49.0, 1101.0, 2000.0, 5000.0]            # unvoiced, below f0_min (index 1), above f0_max (index 255)
    table = rnd(32, 300, C)
    idx64, m = ref64.f0_to_coarse(torch.from_numpy(f0[:, ::2]).double())
    assert float((m - m.round()).abs().min()) >= 1e-3 and idx64.min() == 1 and idx64.max() == 255 and len(idx64.unique()) > 10
    f0_d, table_d = torch.from_numpy(f0).to(DEV), table.to(DEV)

    def run():
        index, y = torch.full((B, T), -1, dtype=torch.int32, device=DEV), torch.empty(B, T, C, device=DEV)
        a2m.pitch_embed(f0_d, B, T, table_d, index, y)
        return index, y
    index, y = run()
    assert torch.equal(index.cpu().long(), idx64)
    assert torch.equal(y.cpu(), table[idx64])
    i2, y2 = run()
    assert torch.equal(i2, index) and torch.equal(y2, y)
