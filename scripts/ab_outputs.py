"""What one build of the library computes -- the head frame (both SR precisions), ray-kernel shapes, the torso frame, the three
token-transformer models, and the launch traces of the frames and the models -- saved so that
`scripts/ab.py outputs A B` can compare two builds (the tolerances and their reasons are in `_ab.compare_outputs`).  `R3D_LIB` selects the
build (default: the tree's own library).  Prints a `digest` line per group of arrays and `time` lines: the head frame on one stream by the
host clock, the ray kernel per shape from the library's own events (`r3d_profile_read`, 20 calls).
The package and bench.py come from PYTHONPATH where it names a tree -- `ab.py outputs` runs THIS file in each side's tree, so a side
that is an older commit needs no copy of it -- and from this file's own tree otherwise.
usage: ab_outputs.py [OUT.npz]"""
import ctypes, hashlib, os, sys, time
sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))          # behind PYTHONPATH
import numpy as np, torch
import bench
from real3dportrait_amd import TriPlaneGenerator, _lib
import _scenes
dev = torch.device("cuda:0")
dig = lambda *ts: hashlib.sha1(b"".join(t.contiguous().cpu().numpy().tobytes() for t in ts)).hexdigest()[:16]
print("lib", _lib.LIB_PATH)
SAVE = {}
# A launch trace: the _lib.counting() list with every address (device pointers, the stream) replaced by the index of its first appearance in the
# trace, a host pointer (a ctypes object) by "host", scalars kept: equal digests mean the same entry points in the same order with the same scalars and the same buffer wiring
def trace(calls):
    first, out = {}, []
    for name, args in calls:
        n, stream, devptrs, _ = _lib._plans[name]
        where = {i for i, _, _ in devptrs} | ({n - 1} if stream else set())
        out.append((name,) + tuple(first.setdefault(a, len(first)) if i in where and a is not None else a if isinstance(a, (int, float, str, bytes, type(None))) else "host"
                                   for i, a in enumerate(args)))
    return out
def fold_trace(frame):
    """r3d_chain_fold takes HOST arrays, which the trace above cannot see into: every fold of one frame as (its ops' scalars and sources, N, the
    bounds it reads, the rows it clears), the device addresses by first appearance over the frame's folds."""
    from real3dportrait_amd import sr_with_ref, superresolution
    first, out, real = {}, [], superresolution.chain_fold
    ix = lambda a: None if a is None else first.setdefault(a, len(first))
    def chain_fold(ops, N, ext, zero=()):
        out.append(([(o.kind, o.Cin, o.Cout, o.ksize, o.act, o.gain, o.clamp, o.src_a, o.src_b, ix(o.scales), ix(o.prepacked), ix(o.bias)) for o in ops], N,
                    [ix(t.data_ptr()) for t in ext], [ix(t.data_ptr()) for t in zero]))
        return real(ops, N, ext, zero=zero)
    superresolution.chain_fold = sr_with_ref.chain_fold = chain_fold
    try:
        frame()
    finally:
        superresolution.chain_fold = sr_with_ref.chain_fold = real
    torch.cuda.synchronize()
    return out
def frame_trace(name, frame):
    """The launch trace of one frame, taken after the frames above warmed every cache."""
    with torch.no_grad(), _lib.counting() as calls:
        frame()
    torch.cuda.synchronize()
    tr = trace(calls)
    print("digest %s trace %s (%d calls)" % (name, hashlib.sha1(repr(tr).encode()).hexdigest()[:16], len(tr)))
    with torch.no_grad():
        folds = fold_trace(frame)
    print("digest %s folds %s (%d folds)" % (name, hashlib.sha1(repr(folds).encode()).hexdigest()[:16], len(folds)))
# 1. the head frame, 4 frames of the clip, both SR precisions
for prec in ("f16mx", "f16x3"):
    G, clip, dec, scene = bench.build_scene(torch, dev, n_frames=8, precision=prec)
    fr = [clip.render_u8(t).clone() for t in range(4)]
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for t in range(40): clip.render_u8(t % 8)
    torch.cuda.synchronize()
    print("digest head_frame %s %s" % (prec, dig(*fr)))
    SAVE["head_frame_" + prec] = torch.stack(fr).cpu().numpy()
    print("time head_frame %s one stream %.4f ms" % (prec, (time.perf_counter() - t0) / 40 * 1e3))
    frame_trace("head_frame " + prec, lambda: clip.render_u8(0))
# 2. ray-kernel shapes (fp32 outputs), then the kernel's own time for the shape
lib = _lib.load()
for (R, Nc, Nf, N) in ((128, 48, 48, 1), (128, 48, 0, 1), (64, 96, 96, 2), (96, 32, 16, 1)):
    call = _scenes.ray_case(R, Nc, Nf, N, seed=77)
    out = call()
    torch.cuda.synchronize()
    print("digest render R=%d %d+%d N=%d %s" % (R, Nc, Nf, N, dig(*out)))
    for nm, t in zip(("rgb", "depth", "wsum"), out[:3]): SAVE["render_R%d_%d+%d_%s" % (R, Nc, Nf, nm)] = t.float().cpu().numpy()
    lib.r3d_profile_configure(1); lib.r3d_profile_reset()
    for _ in range(20): call()
    torch.cuda.synchronize()
    ms, cnt = ctypes.c_double(0), ctypes.c_int(0); lib.r3d_profile_read(0, ctypes.byref(ms), ctypes.byref(cnt)); lib.r3d_profile_configure(0)
    print("time render R=%d %d+%d N=%d kernel %.4f ms" % (R, Nc, Nf, N, ms.value / max(1, cnt.value)))
# 3. the torso frame (fused SuperresolutionHybrid8XDC_Warp forward + to_plane_cnn), f16mx
torch.manual_seed(1234)                          # the generator shell and to_plane_cnn are torch-initialised: same values in both children
G = TriPlaneGenerator().to(dev).eval()
frame, _ = bench.build_torso_frame(torch, dev, G, precision="f16mx")
fr = [frame(t).clone() for t in range(2)]
torch.cuda.synchronize()
print("digest torso_frame f16mx %s" % dig(*fr))
SAVE["torso_frame_f16mx"] = torch.stack(fr).cpu().numpy()
frame_trace("torso_frame f16mx", lambda: frame(2))
# 4. the token-transformer models, seeded synth weights at the goldens' smallest shapes: the output, and the launch trace
from real3dportrait_amd import synth
from real3dportrait_amd.hubert import HubertFeatureModel, hubert_features
from real3dportrait_amd.img2plane import Img2PlaneModel
from real3dportrait_amd.segformer import SegFormerSECC2PlaneBackbone
def token_model(name, model, sd, run):
    own = {k: v for k, v in model.state_dict().items() if k.startswith("low_reso_encoder.")}          # the stand-in's, not synth's
    model.load_state_dict(dict(own, **{k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}), strict=True)
    model.to(dev).eval()
    with torch.no_grad(), _lib.counting() as calls:
        out = run(model)
    torch.cuda.synchronize()
    tr = trace(calls)
    print("digest %s output %s" % (name, dig(out)))
    print("digest %s trace %s (%d calls)" % (name, hashlib.sha1(repr(tr).encode()).hexdigest()[:16], len(tr)))
    SAVE["token_" + name] = out.cpu().numpy()
class StandInEncoder(torch.nn.Module):
    """In the place of DeepLabV3: [B, C, S, S] -> [B, 256, S/8, S/8], the 8 x 8 average pool with channel j % C scaled and shifted by seeded
    constants -- element-wise, so that no library picks an algorithm for it."""
    def __init__(self, seed=70):
        super().__init__()
        self.register_buffer("a", torch.from_numpy(synth.hash_unitvar(seed, (1, 256, 1, 1), stream=4900) * np.float32(2.0)))
        self.register_buffer("b", torch.from_numpy(synth.hash_unitvar(seed, (1, 256, 1, 1), stream=4901) * np.float32(0.5)))
    def forward(self, x):
        p = torch.nn.functional.avg_pool2d(x, 8)
        return p[:, torch.arange(256, device=x.device) % p.shape[1]] * self.a + self.b
uniform = lambda seed, *shape: torch.from_numpy(synth.hash_uniform(seed, int(np.prod(shape)), stream=5).reshape(shape) * np.float32(2.0) - np.float32(1.0)).to(dev)
token_model("secc_1x9x64x64", SegFormerSECC2PlaneBackbone(), synth.synth_secc_backbone(91), lambda m: m.forward_features(uniform(92, 1, 9, 64, 64)))
token_model("img2plane_small_s64", Img2PlaneModel(96, hp={"img2plane_backbone_scale": "small"}, low_reso_encoder=StandInEncoder()),
            synth.synth_img2plane(93, "small", 5, qk_gain=1.5), lambda m: m(uniform(94, 1, 3, 64, 64)))
one_layer = {"hidden_size": 128, "num_hidden_layers": 1, "num_attention_heads": 2, "intermediate_size": 256, "conv_dim": (32,) * 7,
             "num_conv_pos_embeddings": 16, "num_conv_pos_embedding_groups": 4}
token_model("hubert_1layer_n4077", HubertFeatureModel(one_layer), synth.synth_hubert(95, one_layer), lambda m: hubert_features(m, uniform(96, 4077).cpu().numpy() * 0.3))
if len(sys.argv) > 1: np.savez(sys.argv[1], **SAVE)
