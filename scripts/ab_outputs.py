"""What one build of the library computes -- the head frame (both SR precisions), ray-kernel shapes, the torso frame -- saved so that
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
if len(sys.argv) > 1: np.savez(sys.argv[1], **SAVE)
