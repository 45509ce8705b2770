"""GPU: the ray kernel on surface-like scenes (synth.surface_scene: an opaque textured sphere in near-empty space) against a float64
truth -- the reference run in float64 (tests/golden/surface_*.npz) and the double build of the oracle on fresh seeds.

These scenes reach what the diffuse random scenes of test_gpu_parity.py never do: transmittance falling to ~0 at the hit, near-empty
rays with weight sums ~1e-3, importance samples crowded into one or two coarse bins (the sampler's den < 1e-5 branch, the merge's rank
histogram with one bin holding ~Nf samples), alpha rounding to 1 (the dense variant), and -- with injected ties -- the merge's exact
counting sort.  The bound (tests/surface_common.py) is per output and ray class:
err(HIP vs fp64) <= max(tier, 2 x err(fp32 reference vs fp64)); valid exactly equal, every output finite.
"""
import numpy as np
import pytest

import surface_common as sc
from test_gpu_parity import T, hip_render, make_decoder, opts

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from real3dportrait_amd import _lib
    _lib.load()          # raises if the HIP extension is missing: no fallback
    return torch


@pytest.fixture(scope="module")
def oracle64():
    from oracle import Oracle
    return Oracle("f64")


def merge_fallbacks(reset=True):
    """Rays whose merge took the exact counting sort since the last reset (r3d_debug_merge_fallbacks)."""
    import ctypes
    from real3dportrait_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "r3d_debug_merge_fallbacks"), "%s does not export the merge test hook: rebuild it" % _lib.LIB_PATH
    n = ctypes.c_ulonglong(0)
    _lib.check(lib.r3d_debug_merge_fallbacks(ctypes.byref(n), int(reset)), "debug_merge_fallbacks")
    return int(n.value)


def truth_and_fp32_err(oracle, oracle64, planes, dec, o, d, Nc, Nf, noise_c, u_f, box_warp=1.0, white_back=False, D=1):
    """(fp64 oracle outputs, {output: per-class err of the fp32 oracle against them})."""
    args = (planes, dec, o, d, Nc, Nf, noise_c, u_f, box_warp, white_back)
    truth = oracle64.render(*args, triplane_depth=D)
    ref32 = oracle.render(*args, triplane_depth=D)
    assert np.array_equal(truth[3], ref32[3])
    return truth, sc.class_errors(ref32, truth, sc.classes(truth[2]))


# ------------------------------------------------------------------------------------------------
# the reference's float64 goldens
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.SURFACE_CASES)
def test_surface_golden_vs_fp64_reference(torch_cuda, name):
    g = sc.load_surface(name)
    got = hip_render(torch_cuda, g["planes"], g["dec"], g["origins"], g["dirs"], int(g["Nc"]), int(g["Nf"]), g["noise_c"], g["u_f"],
                     float(g["box_warp"]), bool(g["white_back"]), int(g["triplane_depth"]))
    sc.check_bound("hip vs ref64 " + name, got, (g["rgb64"], g["depth64"], g["wsum64"], g["valid"]), g["err_fp32_ref"])


# ------------------------------------------------------------------------------------------------
# fresh seeds against the fp64 oracle
# ------------------------------------------------------------------------------------------------
def _fresh(torch, oracle, oracle64, what, planes, dec, o, d, Nc, Nf, noise_c, u_f, D=1):
    truth, err32 = truth_and_fp32_err(oracle, oracle64, planes, dec, o, d, Nc, Nf, noise_c, u_f, D=D)
    got = hip_render(torch, planes, dec, o, d, Nc, Nf, noise_c, u_f, triplane_depth=D)
    sc.check_bound(what, got, truth, err32)


@pytest.mark.parametrize("Nf", [0, 1, 48, 96])
@pytest.mark.parametrize("Nc", [4, 63, 64, 65, 96])
def test_surface_sample_counts_vs_fp64_oracle(torch_cuda, oracle, oracle64, Nc, Nf):
    """Nc / Nf on both sides of the 64-lane slot boundaries of the coarse and merged passes, Nc = 4 (one cdf bin), Nf = 1."""
    from real3dportrait_amd import synth
    seed, R = 400 + Nc + 7 * Nf, 24
    planes, dec = synth.surface_scene(seed, H=64, W=64)
    cam = synth.look_at_camera(0.1, 0.05)[None]
    o, d = oracle.raygen(cam[:, :16], cam[:, 16:], R)
    noise_c = synth.synth_noise(seed, (1, R * R, Nc, 1), stream=7)
    u_f = synth.synth_noise(seed, (R * R, Nf), stream=8)
    _fresh(torch_cuda, oracle, oracle64, "hip vs orc64 Nc=%d Nf=%d" % (Nc, Nf), planes, dec, o, d, Nc, Nf, noise_c, u_f)


def test_surface_three_cameras_non_square_vs_fp64_oracle(torch_cuda, oracle, oracle64):
    """N = 3 cameras, M = 300 rays each (not a square image: linear ray order), dense variant, 64 + 65 samples."""
    from real3dportrait_amd import synth
    N, R, M, Nc, Nf = 3, 20, 300, 64, 65
    planes, dec = synth.surface_scene(431, N=N, H=48, W=48, dense=True)
    cams = synth.camera_sweep(N, -0.35, 0.3)
    o, d = oracle.raygen(cams[:, :16], cams[:, 16:], R)
    o, d = np.ascontiguousarray(o[:, :M]), np.ascontiguousarray(d[:, :M])
    noise_c = synth.synth_noise(432, (N, M, Nc, 1), stream=7)
    u_f = synth.synth_noise(432, (N * M, Nf), stream=8)
    _fresh(torch_cuda, oracle, oracle64, "hip vs orc64 N=3 M=300", planes, dec, o, d, Nc, Nf, noise_c, u_f)


def test_surface_trigrid_vs_fp64_oracle(torch_cuda, oracle, oracle64):
    """Tri-grid sampling (depth 3) of the surface, N = 2, 48 + 48."""
    from real3dportrait_amd import synth
    N, R, Nc, Nf, D = 2, 20, 48, 48, 3
    planes, dec = synth.surface_scene(441, N=N, H=32, W=32, triplane_depth=D)
    cams = synth.camera_sweep(N, -0.25, 0.3)
    o, d = oracle.raygen(cams[:, :16], cams[:, 16:], R)
    noise_c = synth.synth_noise(442, (N, R * R, Nc, 1), stream=7)
    u_f = synth.synth_noise(442, (N * R * R, Nf), stream=8)
    _fresh(torch_cuda, oracle, oracle64, "hip vs orc64 trigrid D=3", planes, dec, o, d, Nc, Nf, noise_c, u_f, D=D)


@pytest.mark.parametrize("mode", ["rays", "camera"])
def test_surface_hash_noise_vs_fp64_oracle(torch_cuda, oracle, oracle64, mode):
    """noise_mode='hash' (the kernel derives the sampling noise itself; synth.render_hash_noise mirrors it for the oracle), with explicit
    rays and in camera mode (rays generated inside the kernels; the oracle gets RaySampler's rays, bit-identical to that mode)."""
    torch = torch_cuda
    from real3dportrait_amd import ImportanceRenderer, RaySampler, synth
    N, R, Nc, Nf, seed = 2, 24, 48, 48, 451
    planes, dec = synth.surface_scene(seed, N=N, H=64, W=64)
    cams = synth.camera_sweep(N, -0.2, 0.35)
    camt = T(torch, cams)
    c2w, K = camt[:, :16].reshape(-1, 4, 4), camt[:, 16:].reshape(-1, 3, 3)
    o, d = RaySampler()(c2w, K, R)
    ren = ImportanceRenderer(hp={})
    ren.noise_mode, ren.seed = "hash", 987654321
    with torch.no_grad():
        if mode == "rays":
            out = ren(T(torch, planes), make_decoder(torch, dec), o, d, opts(Nc, Nf))
        else:
            out = ren.forward_camera(T(torch, planes), make_decoder(torch, dec), c2w, K, R, opts(Nc, Nf))
    torch.cuda.synchronize()
    got = [t.cpu().numpy() for t in out]
    noise_c, u_f = synth.render_hash_noise(ren.seed, np.arange(N * R * R), Nc, Nf)
    o, d = o.cpu().numpy(), d.cpu().numpy()
    truth, err32 = truth_and_fp32_err(oracle, oracle64, planes, dec, o, d, Nc, Nf, noise_c.reshape(N, R * R, Nc, 1), u_f)
    sc.check_bound("hip vs orc64 hash/" + mode, got, truth, err32)


def test_surface_benchmark_shape_strided_vs_fp64_oracle(torch_cuda, oracle, oracle64):
    """The benchmarked shape -- R = 128, 48 + 48, 256^2 planes, hash noise -- checked on every 4th row and column.  Every ray hits the
    box, so the oracle's run over the subset has the same limits; the global depth clamp only moves non-finite depths, and the
    background density keeps every weight sum > 0."""
    torch = torch_cuda
    from real3dportrait_amd import ImportanceRenderer, RaySampler, synth
    R, Nc, Nf = 128, 48, 48
    planes, dec = synth.surface_scene(461, H=256, W=256)
    cam = synth.look_at_camera(0.12, -0.07)[None]
    camt = T(torch, cam)
    o, d = RaySampler()(camt[:, :16].reshape(-1, 4, 4), camt[:, 16:].reshape(-1, 3, 3), R)
    ren = ImportanceRenderer(hp={})
    ren.noise_mode, ren.seed = "hash", 4242
    with torch.no_grad():
        out = ren(T(torch, planes), make_decoder(torch, dec), o, d, opts(Nc, Nf))
    torch.cuda.synchronize()
    idx = (np.arange(0, R, 4)[:, None] * R + np.arange(0, R, 4)[None, :]).reshape(-1)
    got = [t.cpu().numpy()[:, idx] for t in out]
    assert got[3].all()
    noise_c, u_f = synth.render_hash_noise(ren.seed, idx, Nc, Nf)
    o, d = o.cpu().numpy()[:, idx], d.cpu().numpy()[:, idx]
    truth, err32 = truth_and_fp32_err(oracle, oracle64, planes, dec, o, d, Nc, Nf, noise_c.reshape(1, -1, Nc, 1), u_f)
    sc.check_bound("hip vs orc64 R=128 strided", got, truth, err32)


# ------------------------------------------------------------------------------------------------
# ties: the merge's exact counting sort
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Nc,Nf", [(48, 48), (96, 96)])
def test_surface_tied_fine_samples_take_counting_sort(torch_cuda, oracle, oracle64, Nc, Nf):
    """Exact duplicates among the importance u (a pair, a triple), u = 0.0 twice and u = 1 - 2^-24 twice in every ray: tied fine depths
    collide in the merge's rank fast path and every ray must take the exact counting sort (the debug counter says which path ran).
    Tied samples carry identical features, so the result does not depend on their order and is held to the fp64 bound like any other.
    The untied run takes none: its u are stratified (>= 0.6 / Nf apart).  With plain 24-bit random u, 96 fine samples crowded into
    one bin do land 1 ulp apart, and the kernel's rounding can then tie them (seen at 96 + 96) -- the fallback is a real path."""
    from real3dportrait_amd import synth
    R, seed = 20, 470 + Nc
    planes, dec = synth.surface_scene(seed, H=64, W=64)
    cam = synth.look_at_camera(0.1, 0.05)[None]
    o, d = oracle.raygen(cam[:, :16], cam[:, 16:], R)
    noise_c = synth.synth_noise(seed, (1, R * R, Nc, 1), stream=7)
    j = np.arange(Nf, dtype=np.float32)[None, :]
    u_f = ((j + np.float32(0.2) + np.float32(0.6) * synth.synth_noise(seed, (R * R, Nf), stream=8)) / np.float32(Nf)).astype(np.float32)
    tied = u_f.copy()
    tied[:, 1] = tied[:, 0]
    tied[:, 5] = tied[:, 4] = tied[:, 3]
    tied[:, 6:8] = 0.0
    tied[:, 8:10] = np.float32(1.0 - 2.0 ** -24)
    tied[:, Nf - 1] = tied[:, Nf // 2]
    merge_fallbacks(reset=True)
    hip_render(torch_cuda, planes, dec, o, d, Nc, Nf, noise_c, u_f)
    assert merge_fallbacks(reset=True) == 0
    got = hip_render(torch_cuda, planes, dec, o, d, Nc, Nf, noise_c, tied)
    assert merge_fallbacks(reset=True) == R * R
    truth, err32 = truth_and_fp32_err(oracle, oracle64, planes, dec, o, d, Nc, Nf, noise_c, tied)
    sc.check_bound("hip vs orc64 ties Nc=%d Nf=%d" % (Nc, Nf), got, truth, err32)
