"""Shared pieces of the surface-scene tests (tests/test_oracle_golden.py on the CPU, tests/test_gpu_surface.py on the GPU).

The scenes are synth.surface_scene: an opaque textured sphere in near-empty space, the regime of a trained checkpoint.  The truth
is float64 (the reference run in float64 for the goldens, oracle/r3d_oracle.c built with -DR3D_ORACLE_F64 for fresh seeds).  The
bound follows the conditioning, per output and per ray class (opaque / silhouette / empty by the fp64 weight sum):

    err(fp32 implementation vs fp64)  <=  max(tier, 2 x err(fp32 reference vs fp64))

tier = RGB_TOL for rgb and wsum, DEPTH_TOL for depth (the suite's flat tolerances).  On an empty ray 1 - exp(-sigma delta) with
sigma delta ~ 1e-4 cancels in fp32, and two correct fp32 implementations of the depth differ by up to ~1e-4 there, so a flat tolerance
against an fp32 golden does not test those rays; the fp32 reference's own error against fp64 is the yardstick instead.
"""
import json

import numpy as np

from conftest import load_golden

RGB_TOL, DEPTH_TOL = 2e-4, 1e-4
TIERS = {"rgb": RGB_TOL, "depth": DEPTH_TOL, "wsum": RGB_TOL}
OUTPUTS = ("rgb", "depth", "wsum")
CLASSES = ("opaque", "silhouette", "empty")
SURFACE_CASES = ["surface_a_r64_48p48", "surface_b_n2_r32_96p96", "surface_c_white_bw_r32_32p16", "surface_d_dense_r48_48p48",
                 "surface_e_trigrid_d3_r16_20p12"]


def classes(wsum64):
    """Ray classes by the fp64 weight sum [N, M, 1]: boolean masks [N, M]."""
    w = np.asarray(wsum64, np.float64)[..., 0]
    return {"opaque": w > 0.99, "silhouette": (w >= 0.01) & (w <= 0.99), "empty": w < 0.01}


def _unshuffle(a, shape):
    """Inverse of make_golden.py's byte shuffle ([4, n] uint8 -> float32 array of `shape`)."""
    return np.ascontiguousarray(np.asarray(a, np.uint8).T).view(np.float32).reshape(shape)


def load_surface(name):
    """A surface golden with the scene regenerated: planes, dec, rgb / depth / wsum / valid (fp32 reference), rgb64 / depth64 /
    wsum64 (float64 reference), err_fp32_ref {output: [per class]}."""
    from real3dportrait_amd import synth
    g = load_golden(name)
    N, M = g["cams"].shape[0], int(g["R"]) ** 2
    g["scene"] = json.loads(str(g["scene"]))
    g["planes"], g["dec"] = synth.surface_scene(N=N, **g["scene"])
    Nc, Nf, seed = int(g["Nc"]), int(g["Nf"]), int(g["noise_seed"])
    g["noise_c"] = synth.synth_noise(seed, (N, M, Nc, 1), stream=7)
    g["u_f"] = synth.synth_noise(seed, (N * M, Nf), stream=8)
    g["rgb"] = _unshuffle(g.pop("rgb_shuffled"), (N, M, 32))
    g["rgb64"] = g["rgb"].astype(np.float64) + _unshuffle(g.pop("rgb64_res_shuffled"), (N, M, 32))
    g["depth64"] = g["depth"].astype(np.float64) + g.pop("depth64_res")
    g["wsum64"] = g["wsum"].astype(np.float64) + g.pop("wsum64_res")
    g["err_fp32_ref"] = {o: g["err_fp32_ref"][i] for i, o in enumerate(OUTPUTS)}
    return g


def class_errors(got, truth, cls):
    """{output: [max |got - truth| per class]} (0 for an empty class); got / truth = (rgb, depth, wsum, ...)."""
    out = {}
    for i, o in enumerate(OUTPUTS):
        d = np.abs(np.asarray(got[i], np.float64) - np.asarray(truth[i], np.float64))
        out[o] = np.array([d[cls[c]].max() if cls[c].any() else 0.0 for c in CLASSES])
    return out


def check_bound(what, got, truth, err_fp32, factor=2.0):
    """Assert err(got vs truth) <= max(tier, factor * err_fp32) per output and class, `valid` exactly equal, every output finite.
    got / truth = (rgb, depth, wsum, valid); err_fp32 = {output: [per class]} of an fp32 reference against the same truth.
    Prints the measured table and returns it."""
    assert np.array_equal(np.asarray(got[3], bool), np.asarray(truth[3], bool)), what + ": valid differs"
    for i, o in enumerate(OUTPUTS):
        assert np.isfinite(got[i]).all(), "%s: non-finite %s" % (what, o)
    cls = classes(truth[2])
    err = class_errors(got, truth, cls)
    bad = []
    for o in OUTPUTS:
        for j, c in enumerate(CLASSES):
            bound = max(TIERS[o], factor * float(err_fp32[o][j]))
            line = "%s %-6s %-10s n=%5d err %.2e  fp32-ref err %.2e  bound %.2e" % (what, o, c, int(cls[c].sum()), err[o][j],
                                                                                   err_fp32[o][j], bound)
            print(line)
            if err[o][j] > bound:
                bad.append(line)
    assert not bad, "\n".join(bad)
    return err
