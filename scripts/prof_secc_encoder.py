"""Time the per-frame SECC encoder (SegFormerSECC2PlaneBackbone, mode b0) at B = 1, 512^2, cano_src_tgt, and print one JSON
line: the HIP encoder (prenet + MiT-b0 + head, forward_features) and the HIP backbone including to_plane_cnn, in ms/frame from HIP events
after warm-up; the same math as eager fp32 torch on the same GPU (tests/segformer_ref64.py in float32, what the reference pays); and the
encoder's kernel launches per frame (counted at the C entry points).
    python scripts/prof_secc_encoder.py [iters]"""
import argparse

import _prof

_prof.paths(tests=True)


def timed(fn, iters):
    """Each side on its own, not in alternating blocks: 5 calls of warm-up, then one block of iters calls between two device events."""
    _prof.by_events(fn, 5)
    return _prof.by_events(fn, iters)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("iters", type=int, nargs="?", default=50)
    iters = ap.parse_args().iters
    import numpy as np
    import torch

    import segformer_ref64 as R
    from real3dportrait_amd import _lib, synth
    from real3dportrait_amd.segformer import SegFormerSECC2PlaneBackbone

    def count_launches(m, x):
        """Kernel launches of one forward_features, counted at the r3d_secc_* entry points (embed1 and a conv with a LayerNorm epilogue
        are two launches each)."""
        with _lib.counting() as calls:
            m.forward_features(x)
        return sum(2 if n == "r3d_secc_embed1" or (n == "r3d_secc_conv" and a[11] is not None) else 1 for n, a in calls if n.startswith("r3d_secc_"))

    dev = "cuda:0"
    sd = synth.synth_secc_backbone(11)
    m = SegFormerSECC2PlaneBackbone()
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}, strict=True)
    m = m.to(dev).eval()
    x = (torch.from_numpy(synth.hash_uniform(13, 9 * 512 * 512, stream=5)).view(1, 9, 512, 512) * 2 - 1).to(dev)
    sd_dev = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in sd.items()}
    with torch.no_grad():
        enc = timed(lambda: m.forward_features(x), iters)
        full = timed(lambda: m(x), iters)
        eager = timed(lambda: R.head(sd_dev, R.encoder(sd_dev, x, torch.float32), torch.float32), iters)
        launches = count_launches(m, x)
        e = R.head(sd_dev, R.encoder(sd_dev, x, torch.float32), torch.float32)
        h = m.forward_features(x)
        diff = float((e - h).abs().max() / e.abs().max())
    _prof.emit({"metric": "secc_encoder_b0_512", "B": 1, "H": 512, "W": 512, "hip_encoder_ms": round(enc, 4),
                "hip_backbone_with_to_plane_cnn_ms": round(full, 4), "eager_fp32_torch_encoder_ms": round(eager, 4),
                "speedup_vs_eager": round(eager / enc, 2), "encoder_launches_per_frame": launches,
                "hip_vs_eager_max_rel_diff": diff, "iters": iters}, None, "prof_secc_encoder")


if __name__ == "__main__":
    main()
