"""GPU: the HuBERT feature extractor end to end (real3dportrait_amd/hubert.py) against the goldens of the reference's own
get_hubert_from_16k_speech and against the fp64 restatement (tests/hubert_ref64.py): outputs and taps within 2e-4 of max|ref|.
Batched against single chunks and reruns bit for bit, the launch list, get_hubert on a PCM-16 file and patch_hubert."""
import functools
import wave

import numpy as np
import pytest
import torch

import hubert_common as common
import hubert_ref64 as R64
from real3dportrait_amd import _lib
from real3dportrait_amd.hubert import chunk_plan, get_hubert, hubert_features, patch_hubert

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def case(name):
    """(golden, config, model on the device, waveform, the fp64 restatement's (output, taps)): computed once, shared, left unchanged."""
    torch.set_num_threads(16)
    g, cfg_name, cfg, sd, speech = common.golden_case(name)
    ref64 = R64.features(sd, cfg, torch.from_numpy(speech.astype(np.float32)), chunk_plan(len(speech)), torch.float64)
    return g, cfg, common.hip_model(cfg_name, sd, DEV), speech, ref64


@pytest.mark.parametrize("name", list(common.CASES))
def test_features_against_the_reference_and_fp64(name):
    g, cfg, model, speech, (out64, taps64) = case(name)
    taps = {}
    out = hubert_features(model, speech, taps=taps)
    assert out.shape == g["hubert"].shape and out.is_cuda and out.dtype == torch.float32 and bool(torch.isfinite(out).all())
    errs = {"hubert/golden": common.rel(out.cpu().numpy(), g["hubert"]), "hubert/fp64": common.rel(out.cpu().numpy(), out64.numpy())}
    for k in common.TAPS:
        t = taps[k][0].cpu().numpy()
        assert t.shape == tuple(taps64[k][0].shape), k
        errs[k + "/golden"] = common.rel(common.tap_rows(name, t), g[k])
        errs[k + "/fp64"] = common.rel(t, taps64[k][0].numpy())
    print(name, {k: "%.3g" % v for k, v in errs.items()})
    assert all(e <= common.TOL for e in errs.values()), errs


def test_forward_takes_normalised_batches():
    """forward(input_values [B, n]) on already normalised input: B = 2 equals the two alone bit for bit, and meets the fp64 restatement."""
    g, cfg, model, speech, _ = case("hubert_b_n4077")
    x = torch.from_numpy(speech.astype(np.float32))
    mean, rstd = R64.wave_stats(x.double())
    xn = torch.stack([((x.double() - mean) * rstd).float()[:4000], ((x.double() - mean) * rstd).float()[77:4077]])
    out = model(xn.to(DEV))
    assert out.shape == (2, 12, cfg["hidden_size"])
    for b in range(2):
        assert torch.equal(out[b], model(xn[b:b + 1].to(DEV))[0])
    sd = {k: v.cpu() for k, v in model.state_dict().items()}
    ref = R64.forward(sd, cfg, xn, torch.float64)[0]
    assert common.rel(out.cpu().numpy(), ref.numpy()) <= common.TOL


def test_chunk_batches_and_reruns_are_bit_identical():
    g, cfg, model, speech, _ = case("hubert_a_n330123")
    one = hubert_features(model, speech, chunk_batch=1)
    assert torch.equal(one, hubert_features(model, speech, chunk_batch=4))
    assert torch.equal(one, hubert_features(model, speech, chunk_batch=1))
    # 100-frame clips: ten full chunks and a tail, so batches of four form (4, 4, 2, then the tail alone)
    assert len(chunk_plan(len(speech), 100)) == 11
    short = hubert_features(model, speech, clip_frames=100, chunk_batch=1)
    with _lib.counting() as calls:
        assert torch.equal(short, hubert_features(model, speech, clip_frames=100, chunk_batch=4))
    assert [a[2] for n, a in calls if n == "r3d_hubert_conv0"] == [4, 4, 2, 1]
    assert [a[3:6] for n, a in calls if n == "r3d_hubert_conv0"] == [(0, 32000, 32080), (128000, 32000, 32080), (256000, 32000, 32080), (320000, 32000, 10123)]
    assert short.shape == one.shape


def test_launch_list():
    """the statistics once per clip; per chunk batch conv0, six conv_ln_gelu, the projection, the positional conv, six launches
    a layer, the final LayerNorm."""
    g, cfg, model, speech, _ = case("hubert_a_n330123")
    with _lib.counting() as calls:
        hubert_features(model, speech)
    layer = ["r3d_secc_linear", "r3d_secc_linear", "r3d_i2p_attention", "r3d_secc_linear", "r3d_secc_linear", "r3d_secc_linear"]
    chunk = ["r3d_hubert_conv0"] + ["r3d_hubert_conv_ln_gelu"] * 6 + ["r3d_secc_linear", "r3d_hubert_pos_conv"] \
        + layer * cfg["num_hidden_layers"] + ["r3d_secc_layernorm"]
    assert [n for n, _ in calls] == ["r3d_hubert_wave_stats"] + chunk * 2


def write_pcm16(path, samples, channels=1):
    data = np.round(np.asarray(samples) * 32768).astype("<i2")
    if channels > 1:
        data = np.stack([data] + [np.zeros_like(data)] * (channels - 1), axis=1)
    with wave.open(str(path), "wb") as f:
        f.setnchannels(channels)
        f.setsampwidth(2)
        f.setframerate(16000)
        f.writeframes(data.tobytes())


def test_get_hubert_on_a_pcm16_file_and_patch_hubert(tmp_path):
    g, cfg, model, speech, _ = case("hubert_b_n4077")
    write_pcm16(tmp_path / "a.wav", speech)
    write_pcm16(tmp_path / "stereo.wav", speech, channels=2)
    want = hubert_features(model, speech).cpu().numpy()
    got = get_hubert(model, str(tmp_path / "a.wav"))
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == (16, cfg["hidden_size"])
    assert np.array_equal(got[:12], want) and not got[12:].any()
    assert np.array_equal(get_hubert(model, str(tmp_path / "stereo.wav")), got)          # the first channel is taken

    class Infer:
        def get_hubert(self, wav16k_name):
            return "reference"

    infer = Infer()
    assert patch_hubert(infer, model) is True
    assert np.array_equal(infer.get_hubert(str(tmp_path / "a.wav")), got)
    assert infer._r3d_reference_get_hubert("x") == "reference"
    patch_hubert(infer, model)                                                           # a second patch keeps the reference's method
    assert infer._r3d_reference_get_hubert("x") == "reference"
