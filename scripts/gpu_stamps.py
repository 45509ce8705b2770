"""Per-phase s_memtime cycle split of a kernel from an instrumented build (make EXTRA=-DR3D_STAMPS OUT=../lib/libr3d_hip_stamps.so
OBJDIR=../lib/obj_stamps; run with R3D_LIB=.../libr3d_hip_stamps.so).  The stamp readers r3d_debug_stamps / r3d_debug_stamps_sr exist in
that build only, so they are bound here and not in _lib.py.
usage: gpu_stamps.py up [PREC=f16x3]      the fused up-sampling conv and the conv1 after it: block0 (32 -> 256, 128^2 -> 256^2) and block1
                                          (256 -> 128, 256^2 -> 512^2), mean cycles per WAVE
       gpu_stamps.py wino [PREC=f16mx]    the Winograd F(2,3) conv1 of the same two blocks (run with R3D_CONV_WINO=1), mean cycles per WAVE
       gpu_stamps.py ray [R=128 Nc=48 Nf=48]   the fused ray kernel, mean cycles per ray (wave time; two waves share a SIMD)"""
import ctypes, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from real3dportrait_amd import _lib
import _scenes

# phase names per mode, in the order of the stamp slots (csrc/r3d_stamps.h)
PHASES = {"up": ["prologue", "main loop: compute", "FIR epilogue", "store drain", "main loop: own DMA wait", "main loop: barrier"],
          "up conv1": ["prologue", "main loop", "epilogue", "store drain"],
          "wino": ["prologue", "matrix phase", "transform phase", "drain (vmcnt/lgkmcnt) before barrier", "barrier", "exchange", "epilogue", "store drain"],
          "ray": ["setup+depths", "coarse decode", "march+importance", "fine decode", "merge", "final march+omega", "composite+store", "between rays",
                  "coarse gather", "fine gather"]}
BLOCKS = ((32, 256, 128, 100), (256, 128, 256, 200))          # cin, cout, input side, weight seed

mode, args = (sys.argv[1] if len(sys.argv) > 1 else ""), sys.argv[2:]
if mode not in ("up", "wino", "ray"): sys.exit(__doc__)
lib = ctypes.CDLL(_lib.LIB_PATH)
buf = (ctypes.c_ulonglong * 32)()


def rows(row, names, base, per):
    """One row per phase, slots base.. of the stamps: mean cycles per wave / ray and the share of the phases' sum."""
    tot = sum(buf[base + i] for i in range(len(names)))
    for i, n in enumerate(names):
        print(row % (n, buf[base + i] / max(1, per), 100.0 * buf[base + i] / max(1, tot)))


def clock_line(text, slot):
    """The shader clock the waves ran at: s_memtime cycles / s_memrealtime ticks x the wall-clock rate (100 MHz on gfx950)."""
    hip = ctypes.CDLL("libamdhip64.so"); wr = ctypes.c_int(0); hip.hipDeviceGetAttribute(ctypes.byref(wr), 10017, 0)   # hipDeviceAttributeWallClockRate (kHz)
    wr_khz = wr.value if wr.value > 0 else 100000
    if buf[slot + 1]: print(text % {"ghz": buf[slot] / buf[slot + 1] * wr_khz / 1e6, "khz": wr_khz})


if mode == "ray":
    R, Nc, Nf = (int(args[i]) if len(args) > i else v for i, v in enumerate((128, 48, 48)))
    call = _scenes.ray_case(R, Nc, Nf, need_depth=False)
    for _ in range(3): call()
    torch.cuda.synchronize()
    assert lib.r3d_debug_stamps(buf) == 0
    reps = 10
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    for _ in range(reps): call()
    ev1.record(); torch.cuda.synchronize()
    assert lib.r3d_debug_stamps(buf) == 0
    rays, tot = buf[31], sum(buf[i] for i in range(10))
    print("R=%d %d+%d: %.3f ms per call (instrumented), %d rays, %.0f cycles per ray" % (R, Nc, Nf, ev0.elapsed_time(ev1) / reps, rays // reps, tot / rays))
    rows("  %-22s %8.0f cycles  %5.1f %%", PHASES["ray"], 0, rays)
    clock_line("  the waves ran at %(ghz).3f GHz (s_memtime cycles / s_memrealtime ticks x 100 MHz)", 28)
    sys.exit(0)

prec = args[0] if args else {"up": "f16x3", "wino": "f16mx"}[mode]
for (cin, cout, res, seed) in BLOCKS:
    call = _scenes.sr_block(cin, cout, res, seed, prec)
    for _ in range(2): call()
    torch.cuda.synchronize(); assert lib.r3d_debug_stamps_sr(buf) == 0
    reps = 5
    for _ in range(reps): call()
    torch.cuda.synchronize(); assert lib.r3d_debug_stamps_sr(buf) == 0
    waves, cw = buf[31], buf[30]          # waves of the up-sampling conv / of conv1 since the last read
    ctot = sum(buf[12 + i] for i in range(len(PHASES["up conv1" if mode == "up" else "wino"])))
    if mode == "up":
        tot = sum(buf[i] for i in range(6))
        print("up-conv %d -> %d at %d^2 (%s): %d waves per launch, %.0f cycles per wave" % (cin, cout, res, prec, waves // reps, tot / max(1, waves)))
        rows("  %-24s %8.0f cycles  %5.1f %%", PHASES["up"], 0, waves)
        print("  conv1 %d -> %d at %d^2: %d waves per launch, %.0f cycles per wave" % (cout, cout, 2 * res, cw // reps, ctot / max(1, cw)))
        rows("    %-14s %8.0f cycles  %5.1f %%", PHASES["up conv1"], 12, cw)
        for nm, slot in (("up-conv", 28), ("conv1", 26)):
            clock_line("  " + nm + " waves ran at %(ghz).3f GHz (s_memtime / s_memrealtime, wall clock %(khz)d kHz)", slot)
    else:
        print("conv1 %d -> %d at %d^2 (%s, wino=%s): %d waves per launch, %.0f cycles per wave" % (cout, cout, 2 * res, prec, os.environ.get("R3D_CONV_WINO"), cw // reps, ctot / max(1, cw)))
        rows("    %-38s %8.0f cycles  %5.1f %%", PHASES["wino"], 12, cw)
        clock_line("    waves ran at %(ghz).3f GHz", 26)
