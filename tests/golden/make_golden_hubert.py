"""Regenerate the hubert_* golden vectors: the reference's own get_hubert_from_16k_speech (data_gen/utils/process_audio/extract_hubert.py:18-80)
on CPU in fp32, with its module globals set: `hubert_model` a transformers.HubertModel built from a HubertConfig with the synthetic weights
of real3dportrait_amd.synth.synth_hubert, `wav2vec2_processor` a small callable around Wav2Vec2FeatureExtractor(do_normalize=True).

Run in the build container only (needs the reference tree, R3D_REFERENCE, and transformers):
    python tests/golden/make_golden_hubert.py
Weights and waveforms are regenerated from the seeds of hubert_common.CASES, so the fixtures hold only outputs.

The reference module imports soundfile, which is not installed: a stand-in goes into sys.modules, AFTER the transformers classes are
imported (transformers' own availability probe raises on a module without a spec).

Stored per case: `hubert` [T, hidden], the reference's chunk list `chunks` [n, 2] (start, end: read off the views it hands the model), four
sub-sampled taps of the first chunk (hubert_common.TAPS, tap_rows), and `attention` [n, 2]: per attention its number of keys L and the median
over query rows of the largest softmax probability, which the maker requires to lie in (2 / L, 0.9), measured by the fp64 restatement
(tests/hubert_ref64.py), which the maker also requires to meet the reference within 2e-4 of max|ref|.  On every model it builds, the maker
runs HubertFeatureModel.from_reference and a strict key comparison."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("R3D_REFERENCE", "/root/reference")
sys.path.insert(0, REF)
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, HERE)

import hubert_common as common  # noqa: E402
import hubert_ref64 as R64  # noqa: E402
from real3dportrait_amd.hubert import HubertFeatureModel, chunk_plan  # noqa: E402


def reference_module():
    from transformers import HubertConfig, HubertModel, Wav2Vec2FeatureExtractor          # before the soundfile stand-in
    if "soundfile" not in sys.modules:
        sys.modules["soundfile"] = types.ModuleType("soundfile")
    import ref_stubs
    ref_stubs.install()
    import data_gen.utils.process_audio.extract_hubert as ref
    fe = Wav2Vec2FeatureExtractor(feature_size=1, sampling_rate=16000, padding_value=0.0, do_normalize=True, return_attention_mask=False)
    ref.wav2vec2_processor = lambda speech, return_tensors="pt", sampling_rate=16000: fe(speech, return_tensors=return_tensors,
                                                                                       sampling_rate=sampling_rate)
    return ref, HubertConfig, HubertModel


def reference_model(HubertConfig, HubertModel, cfg, sd):
    c = HubertConfig(feat_extract_norm="layer", do_stable_layer_norm=True, feat_proj_layer_norm=True, conv_bias=True, hidden_act="gelu",
                     feat_extract_activation="gelu", **{k: (list(v) if isinstance(v, tuple) else v) for k, v in cfg.items()})
    m = HubertModel(c).eval()
    assert sorted(m.state_dict()) == sorted(sd), set(m.state_dict()) ^ set(sd)
    m.load_state_dict(sd, strict=True)
    return m


def check_from_reference(m):
    hip = HubertFeatureModel.from_reference(m)
    want, got = m.state_dict(), hip.state_dict()
    assert list(want) != [] and sorted(want) == sorted(got) and all(torch.equal(got[k], v) for k, v in want.items())
    assert not hip.training


@torch.no_grad()
def run(ref, m, speech):
    """(hubert [T, hidden], taps of the first chunk, the (start, end) of every chunk): hooks on the reference model's own modules."""
    got, chunks, hooks = {}, [], []
    def first(name, fn):          # keeps the first call's output; returns None, so the module's output stays what it is
        def hook(mod, inp, out):
            if name not in got:
                got[name] = fn(out[0] if isinstance(out, tuple) else out)
        return hook

    hooks.append(m.feature_extractor.register_forward_pre_hook(
        lambda mod, inp: chunks.append((inp[0].storage_offset(), inp[0].storage_offset() + inp[0].shape[1])) and None))
    hooks.append(m.feature_extractor.register_forward_hook(first("extract_features", lambda t: t.transpose(1, 2)[0].clone())))
    hooks.append(m.feature_projection.register_forward_hook(first("projected", lambda t: t[0].clone())))
    hooks.append(m.encoder.pos_conv_embed.register_forward_hook(first("pos_embed", lambda t: t[0].clone())))
    hooks.append(m.encoder.layers[0].register_forward_hook(first("layer0", lambda t: t[0].clone())))
    ref.hubert_model = m
    out = ref.get_hubert_from_16k_speech(speech, device="cpu")
    for h in hooks:
        h.remove()
    got["pos_conv"] = got["projected"] + got.pop("pos_embed")          # HubertEncoderStableLayerNorm.forward: hidden + position_embeddings
    return out, got, chunks


def main():
    torch.set_num_threads(16)
    ref, HubertConfig, HubertModel = reference_module()
    keys = {}
    for name, (cfg_name, n, seed_w, seed_x, step) in common.CASES.items():
        cfg_name, cfg, sd, speech = common.case_inputs(name)
        m = reference_model(HubertConfig, HubertModel, cfg, sd)
        check_from_reference(m)
        keys.setdefault(cfg_name, np.array(sorted(m.state_dict())))
        keys.setdefault(cfg_name + ".shapes", np.array([list(m.state_dict()[k].shape) + [0] * (3 - m.state_dict()[k].dim()) for k in sorted(m.state_dict())],
                                                       np.int64))
        hubert, taps, chunks = run(ref, m, speech)
        assert chunks == chunk_plan(n), (chunks, chunk_plan(n))
        assert hubert.shape == ((n - 80) // 320, cfg["hidden_size"])
        stats = []
        wave = torch.from_numpy(speech.astype(np.float32))
        h64, t64 = R64.features(sd, cfg, wave, chunks, torch.float64, stats)
        errs = {"hubert": common.rel(h64.numpy(), hubert.numpy())}
        errs.update({k: common.rel(t64[k][0].numpy(), taps[k].numpy()) for k in common.TAPS})
        assert all(e <= common.TOL for e in errs.values()), (name, errs)
        for L, med in stats:
            assert 2.0 / L < med < 0.9, (name, L, med)
        assert all(float(taps[k].abs().max()) > 0 for k in common.TAPS)
        out = {"spec": np.array([seed_w, seed_x, n], np.int64), "config": np.array(cfg_name), "qk_gain": np.array(common.QK_GAIN),
               "chunks": np.array(chunks, np.int64), "attention": np.array(stats, np.float64), "hubert": hubert.numpy()}
        for k in common.TAPS:
            out[k] = np.ascontiguousarray(common.tap_rows(name, taps[k].numpy()))
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **out)
        print("%s: %d bytes, T %d, chunks %s, fp64 restatement vs reference %s, attention (L, median max p) %s, max|hubert| %.3g"
              % (name, os.path.getsize(path), hubert.shape[0], chunks, {k: "%.2g" % v for k, v in errs.items()},
                 [(L, round(med, 3)) for L, med in stats], float(hubert.abs().max())))
    np.savez_compressed(os.path.join(HERE, "hubert_keys.npz"), **keys)


if __name__ == "__main__":
    main()
