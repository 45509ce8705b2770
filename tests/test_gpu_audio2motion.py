"""GPU: the audio-to-motion VAE (real3dportrait_amd/audio2motion.py) against the goldens of the reference's own classes
(tests/golden/make_golden_audio2motion.py) and against the fp64 restatement (tests/audio2motion_ref64.py), within 2e-4 of max|ref|, and
the host contract around it: launch count, no torch convolution or linear, samples independent of the batch, buffers made once, the
patch."""
import os
import re

import numpy as np
import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

import abi
import audio2motion_ref64 as ref64
from conftest import ROOT, load_golden
from real3dportrait_amd import _lib, synth
from real3dportrait_amd import audio2motion as a2m

pytestmark = pytest.mark.gpu
TOL = 2e-4
DEV = "cuda:0"
HP = synth.AUDIO2MOTION_HPARAMS
CASES = ["pitch_t4", "pitch_b2", "pitch_t2r", "pitch_tr", "vae_t20"]
_models, _cases = {}, {}


def model(pitch):
    """One model per kind for the whole file (the synthetic weights of the goldens), on the GPU; never modified."""
    if pitch not in _models:
        sd = synth.synth_audio2motion(41, pitch)
        m = a2m.PitchContourVAEModel(HP) if pitch else a2m.VAEModel()
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
        _models[pitch] = (sd, m.to(DEV).eval())
    return _models[pitch]


def case(name):
    """golden, batch (numpy), the fp64 restatement's output and taps: computed once and shared."""
    if name not in _cases:
        g = load_golden("audio2motion_" + name)
        pitch, B, T = (int(v) for v in g["shape"])
        assert int(g["seeds"][0]) == 41
        batch = synth.synth_audio2motion_inputs(int(g["seeds"][1]), B, T)
        if not pitch:
            batch = {k: batch[k] for k in ("audio", "y_mask")}
        taps = {}
        x64 = ref64.forward(model(bool(pitch))[0], batch, g["z_p"], bool(pitch), HP, torch.float64, taps=taps)
        _cases[name] = (g, bool(pitch), batch, x64, taps)
    return _cases[name]


def tensors(batch, dev=DEV):
    return {k: torch.from_numpy(v).to(dev) for k, v in batch.items()}


def rel(got, ref):
    ref = torch.as_tensor(ref).double()
    return float((got.double().cpu() - ref).abs().max()) / float(ref.abs().max())


@pytest.mark.parametrize("name", CASES)
def test_golden_case(name):
    g, pitch, batch, x64, _ = case(name)
    m = model(pitch)[1]
    ret = {}
    torch.manual_seed(int(g["seeds"][2]))          # the latent is the reference's draw under the golden's seed
    x = m.forward(tensors(batch), ret, train=False, temperature=1.0)
    assert x.shape == g["out"].shape and x.dtype == torch.float32 and x.device.type == "cuda"
    assert ret["pred"] is x and torch.equal(ret["mask"].cpu(), torch.from_numpy(batch["y_mask"]))
    e_gold, e_64 = rel(x, g["out"]), rel(x, x64)
    print("audio2motion %s: %.2e of max|ref| against the golden, %.2e against fp64" % (name, e_gold, e_64))
    assert e_gold <= TOL and e_64 <= TOL
    x2 = m.forward(tensors(batch, "cpu"), {}, z_p=torch.from_numpy(g["z_p"]))          # z_p= supplies the same draw; CPU inputs are moved
    assert torch.equal(x2, x)
    zero = batch["y_mask"] == 0
    assert bool((x.cpu()[torch.from_numpy(zero)] == 0).all())
    xt = m.forward(tensors(batch), {}, z_p=torch.from_numpy(g["z_p"]), temperature=0.5)
    x64t = ref64.forward(model(pitch)[0], batch, g["z_p"], pitch, HP, torch.float64, temperature=0.5)
    assert rel(xt, x64t) <= TOL and rel(xt, x64) > 100 * TOL


def test_intermediates_after_each_flow():
    g, pitch, batch, x64, t64 = case("pitch_b2")
    taps = {}
    model(pitch)[1].forward(tensors(batch), {}, z_p=torch.from_numpy(g["z_p"]), _taps=taps)
    assert torch.equal(taps["pitch_index"].cpu().long(), t64["pitch_index"])
    names = ["cond_feat", "g_sqz"] + ["z_flow%d" % i for i in (3, 2, 1, 0)] + ["dec_in"] + ["dec_x%d" % i for i in range(3)] + ["dec_out%d" % i for i in range(4)]
    for n in names:
        e = rel(taps[n], t64[n])
        print("audio2motion intermediate %-9s %.2e of max|ref|" % (n, e))
        assert e <= TOL, (n, e)
    # the flows do something, each of them
    z = [torch.from_numpy(g["z_p"]).transpose(1, 2).double()] + [t64["z_flow%d" % i] for i in (3, 2, 1, 0)]
    assert all(float((a.flip(2) - b).abs().max()) > 0.05 and float((a - b).abs().max()) > 0.05 for a, b in zip(z[:-1], z[1:]))


@pytest.mark.parametrize("name", ["pitch_b2", "vae_t20"])
def test_launches_and_no_torch_layers(name):
    g, pitch, batch, _, _ = case(name)
    m, b = model(pitch)[1], tensors(batch)
    z_p = torch.from_numpy(g["z_p"])
    m.forward(b, {}, z_p=z_p)

    class Ops(TorchDispatchMode):
        seen = []

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            self.seen.append(str(func))
            return func(*args, **(kwargs or {}))
    with _lib.counting() as calls, Ops() as ops:
        m.forward(b, {}, z_p=z_p)
    names = [c[0] for c in calls]
    want = a2m.LAUNCHES_PITCH if pitch else a2m.LAUNCHES_VAE
    assert len(names) == want == (37 if pitch else 33)
    assert names.count("r3d_a2m_wn_layer") == 20 and names.count("r3d_a2m_pitch_embed") == int(pitch) and set(names) <= set(abi.header_declarations("r3d_hip_audio.h"))
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = design[design.index("### 4.20"):]
    assert re.search(r"\b%d launches\b" % want, sec), "DESIGN 4.20 does not state %d launches" % want
    bad = [o for o in ops.seen if re.search(r"conv|linear|addmm|\bmm\b|bmm|matmul|batch_norm|gelu|tanh|sigmoid|embedding", o)]
    assert not bad, bad


def test_sample_of_a_batch_equals_the_sample_alone():
    g, pitch, batch, _, _ = case("pitch_b2")
    m = model(pitch)[1]
    x = m.forward(tensors(batch), {}, z_p=torch.from_numpy(g["z_p"]))
    for b in (0, 1):
        one = {k: v[b:b + 1] for k, v in batch.items()}
        xb = m.forward(tensors(one), {}, z_p=torch.from_numpy(g["z_p"][b:b + 1]))
        assert torch.equal(xb[0], x[b]), b
    assert not torch.equal(x[0], x[1])


def test_second_call_allocates_no_buffer_and_folds_nothing():
    g, pitch, batch, _, _ = case("pitch_tr")
    sd = model(pitch)[0]
    m = a2m.PitchContourVAEModel(HP)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    m = m.to(DEV).eval()
    b, z_p = tensors(batch), torch.from_numpy(g["z_p"])
    x1 = m.forward(b, {}, z_p=z_p)
    bufs = dict(m._buffers_for(torch.device(DEV), 1, batch["y_mask"].shape[1]))
    ptrs = {k: v.data_ptr() for k, v in bufs.items()}
    folds, gen, n = m._prepare(), m._derived.generation, len(m._work)
    x2 = m.forward(b, {}, z_p=z_p)
    after = m._buffers_for(torch.device(DEV), 1, batch["y_mask"].shape[1])
    assert len(m._work) == n == 1 and all(after[k] is bufs[k] and after[k].data_ptr() == ptrs[k] for k in bufs)
    assert m._prepare() is folds and m._derived.generation == gen == 1
    assert torch.equal(x1, x2) and x1.data_ptr() != x2.data_ptr()          # the result is the caller's, not a work buffer
    with torch.no_grad():                                                  # a changed parameter is folded again
        m.vae.decoder.out_proj.bias.add_(0.5)
    x3 = m.forward(b, {}, z_p=z_p)
    assert m._derived.generation == 2 and rel(x3, x1.cpu() + 0.5) <= 1e-6


def test_a_batch_without_blink_and_amplitude_takes_the_references_defaults():
    g, pitch, batch, _, _ = case("pitch_tr")
    m, sd = model(pitch)[1], model(pitch)[0]
    bare = {k: batch[k] for k in ("audio", "f0", "y_mask")}
    b = tensors(bare)
    x = m.forward(b, {}, z_p=torch.from_numpy(g["z_p"]))
    assert b["blink"].shape == (1, batch["f0"].shape[1], 1) and b["blink"].dtype == torch.long          # vae.py:404-405 adds it to the batch
    full = dict(bare, blink=np.zeros_like(batch["blink"]), mouth_amp=np.full((1, 1), 0.4, np.float32))
    x64 = ref64.forward(sd, full, g["z_p"], True, HP, torch.float64)
    assert rel(x, x64) <= TOL
    with pytest.raises(ValueError, match="multiple of 4"):
        m.forward(tensors({k: v[:, :-2] if k != "y_mask" else v[:, :-1] for k, v in bare.items()}), {})


def test_patch_audio2secc_on_a_stub():
    recorded = sorted(str(k) for k in load_golden("audio2motion_keys")["pitch"])

    class PitchContourVAEModel(a2m.PitchContourVAEModel):          # stands for the reference's class: its name, another module
        pass
    sd, _ = model(True)
    ref = PitchContourVAEModel(HP)
    ref.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    assert sorted(ref.state_dict()) == recorded
    ref = ref.to(DEV).train()

    class Infer:
        pass
    infer = Infer()
    infer.audio2secc_model = ref
    assert a2m.patch_audio2secc(infer) is True
    new = infer.audio2secc_model
    assert type(new) is a2m.PitchContourVAEModel and infer._r3d_reference_audio2secc_model is ref and not new.training
    assert new.device == ref.device and new.hparams == ref.hparams
    assert a2m.patch_audio2secc(infer) is False and infer.audio2secc_model is new
    g, _, batch, x64, _ = case("pitch_t4")
    ret = {}
    pred = new.forward(tensors(batch), ret=ret, train=False, temperature=1.0, z_p=torch.from_numpy(g["z_p"]))          # real3d_infer.py:369
    assert rel(ret["pred"], x64) <= TOL and pred.shape[-1] == 64
