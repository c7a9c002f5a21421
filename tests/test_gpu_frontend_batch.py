"""`EngineFrontend.speaker_bundles` / `emo_conds` on the GPU: three WAV prompts of different lengths and sample rates -- one shorter than a second,
with an odd Kaldi frame count -- through ONE ragged prompt-side pass (one feature-extractor call, one w2v-bert pass, one `CAMPPlus.forward_ragged`,
one regulator call), each bundle held to the ORACLE chain on its own file with the gates of tests/test_gpu_frontend.py: `ref_mel` within 5e-4, the three
network outputs within 1e-4 of their largest value.  A synthetic checkpoint directory with the reference's file layout is written here (small w2v-bert /
regulator widths, the real CAMPPlus architecture, oracle-seeded weights).

An odd frame count leaves half a pair of frames: the feature extractor pads it, the attention mask drops it, and the engine returns that row as the
hidden state 0 normalised ((0 - mean) / std, `Wav2Vec2BertModel._pad`), where the oracle's class leaves whatever the network computes on padding.
`spk_cond_emb` is therefore compared on the valid rows (as test_gpu_frontend.py compares the emotion prompt), and the oracle regulator reads the
oracle's embedding with that one row set to the engine's convention."""
import json

import numpy as np
import pytest
import torch

from oracle import audio_oracle as AO
from oracle import campplus_oracle as CO
from oracle import codec_oracle as KO
from oracle import w2vbert_oracle as WO
from tools.make_golden_audio import speechlike

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WCFG = WO.W2VBertCfg(hidden_size=64, num_hidden_layers=4, num_attention_heads=2, intermediate_size=128, feature_projection_input_dim=160,
                     left_max_position_embeddings=6, right_max_position_embeddings=2, conv_depthwise_kernel_size=7)
RCFG = KO.RegulatorConfig(channels=64, in_channels=64, n_layers=4, groups=1, codebook_size=64)
CLIPS = (("a.wav", 24000, 48000, 71), ("b.wav", 32000, 22720, 72), ("c.wav", 24000, 31000, 73))      # (file, rate, samples, seed): 2 s, 0.71 s, 1.29 s


def write_batch_checkpoint_dir(d):
    from safetensors.torch import save_file
    from scipy.io import wavfile
    g = torch.Generator().manual_seed(15)
    wdir = d / "hf_cache" / "w2v-bert-2.0"
    wdir.mkdir(parents=True)
    (wdir / "config.json").write_text(json.dumps(dict(
        hidden_size=WCFG.hidden_size, num_hidden_layers=WCFG.num_hidden_layers, num_attention_heads=WCFG.num_attention_heads,
        intermediate_size=WCFG.intermediate_size, feature_projection_input_dim=WCFG.feature_projection_input_dim,
        position_embeddings_type="relative_key", left_max_position_embeddings=WCFG.left_max_position_embeddings,
        right_max_position_embeddings=WCFG.right_max_position_embeddings, conv_depthwise_kernel_size=WCFG.conv_depthwise_kernel_size,
        hidden_act="swish", layer_norm_eps=WCFG.layer_norm_eps, add_adapter=False, model_type="wav2vec2-bert", vocab_size=None)))
    wsd = WO.synth_weights(WCFG)
    save_file({k: v.contiguous() for k, v in wsd.items()}, str(wdir / "model.safetensors"))
    stats = {"mean": 0.3 * torch.randn(WCFG.hidden_size, generator=g), "var": 0.5 + torch.rand(WCFG.hidden_size, generator=g)}
    torch.save(stats, d / "wav2vec2bert_stats.pt")
    csd = CO.synth_weights()
    torch.save(csd, d / "hf_cache" / "campplus_cn_common.bin")
    rsd = KO.synth_regulator_weights(RCFG, 9)
    torch.save({"net": {"cfm": {"module.placeholder": torch.zeros(1)}, "length_regulator": {"module." + k: v for k, v in rsd.items()}}}, d / "s2mel.pth")
    torch.save({"model": {"up.bias": torch.zeros(4)}}, d / "codec.pth")
    for name, rate, n, seed in CLIPS:
        wavfile.write(str(d / name), rate, np.round(speechlike(n, rate, seed) * 32767.0).astype(np.int16))
    cfg = {"w2v_stat": "wav2vec2bert_stats.pt", "s2mel_checkpoint": "s2mel.pth",
           "s2mel": {"length_regulator": {"channels": RCFG.channels, "sampling_ratios": [1, 1, 1, 1], "is_discrete": False,
                                          "in_channels": RCFG.in_channels, "content_codebook_size": RCFG.codebook_size},
                     "preprocess_params": {"sr": 22050, "spect_params": {"n_fft": 1024, "win_length": 1024, "hop_length": 256, "n_mels": 80,
                                                                         "fmin": 0, "fmax": "None"}}}}
    return cfg, dict(wsd=wsd, stats=stats, csd=csd, rsd=rsd)


def _oracle_emb(w, a16):
    """-> (emb (1, ceil(F / 2), D) with a padded half pair's row in the engine's convention, valid rows mask)"""
    feats, mask = AO.seamless_features(a16[0].numpy())
    mean, std = w["stats"]["mean"], torch.sqrt(w["stats"]["var"])
    emb = WO.get_emb(w["wsd"], WCFG, torch.from_numpy(feats), torch.from_numpy(mask).long(), mean, std, layer=WCFG.num_hidden_layers)
    valid = torch.from_numpy(mask[0]).bool()
    emb = emb.clone()
    emb[0, ~valid] = (0.0 - mean) / std
    return emb, valid


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    from indextts_amd.frontend import EngineFrontend, load_wav
    d = tmp_path_factory.mktemp("batch") / "ckpt"
    cfg, w = write_batch_checkpoint_dir(d)
    fe = EngineFrontend(cfg, str(d), DEV)
    paths = [str(d / c[0]) for c in CLIPS]
    waves = [load_wav(p) for p in paths]
    return fe, paths, waves, w


def test_speaker_bundles_vs_oracle_chain(setup):
    fe, paths, waves, w = setup
    bundles = fe.speaker_bundles(paths)
    assert len(bundles) == len(paths)
    odd = 0
    for p, (x, sr), b in zip(paths, waves, bundles):
        a22 = AO.resample(x, sr, 22050)
        a16 = AO.resample(a22, 22050, 16000)
        emb, valid = _oracle_emb(w, a16)
        odd += int(not bool(valid.all()))
        mel = AO.mel_spectrogram(a22)
        fb = AO.kaldi_fbank(a16)
        style = CO.campplus(w["csd"], (fb - fb.mean(dim=0, keepdim=True))[None])
        cond, _ = KO.length_regulator(w["rsd"], RCFG, emb, torch.tensor([mel.shape[2]]))
        assert b["spk_cond_emb"].shape == emb.shape and b["ref_mel"].shape == mel.shape and b["style"].shape == (1, 192)
        assert b["prompt_condition"].shape == cond.shape == (1, mel.shape[2], RCFG.channels)
        err = dict(spk_cond_emb=float((b["spk_cond_emb"].cpu() - emb)[0, valid].abs().max()), ref_mel=float((b["ref_mel"].cpu() - mel).abs().max()),
                   style=float((b["style"].cpu() - style).abs().max()), prompt_condition=float((b["prompt_condition"].cpu() - cond).abs().max()))
        print(f"speaker_bundles[{p.rsplit('/', 1)[-1]}: {x.shape[1] / sr:.2f} s, {emb.shape[1]} frames] vs the oracle chain, max|d|:",
              {k: f"{v:.2e}" for k, v in err.items()},
              "| scales:", f"emb {float(emb.abs().max()):.1f}, style {float(style.abs().max()):.1f}, cond {float(cond.abs().max()):.1f}")
        assert err["ref_mel"] <= 5e-4
        assert err["spk_cond_emb"] <= 1e-4 * float(emb.abs().max()) and err["style"] <= 1e-4 * float(style.abs().max())
        assert err["prompt_condition"] <= 1e-4 * float(cond.abs().max())
        # keys, shapes, dtypes, devices of the bundle the prompt gets alone
        alone = fe.speaker_bundle(p)
        assert set(b) == set(alone)
        for k in alone:
            assert b[k].shape == alone[k].shape and b[k].dtype == alone[k].dtype and b[k].device == alone[k].device and b[k].is_contiguous(), k
        print("   batched vs alone, max|d|:", {k: f"{float((b[k] - alone[k]).abs().max()):.2e}" for k in alone})
    assert min(x.shape[1] / sr for x, sr in waves) < 1.0 and odd >= 1           # a clip under a second; a padded half pair among the clips


def test_one_prompt_and_no_prompt(setup):
    fe, paths, _, _ = setup
    assert fe.speaker_bundles([]) == [] and fe.emo_conds([]) == []
    one, alone = fe.speaker_bundles(paths[1:2]), fe.speaker_bundle(paths[1])
    assert len(one) == 1 and set(one[0]) == set(alone)
    for k in alone:
        assert one[0][k].shape == alone[k].shape and one[0][k].dtype == alone[k].dtype
        assert float((one[0][k] - alone[k]).abs().max()) <= 1e-4 * float(alone[k].abs().max())


def test_emo_conds_vs_oracle_chain(setup):
    fe, paths, waves, w = setup
    es = fe.emo_conds(paths)
    assert len(es) == len(paths)
    for p, (x, sr), e in zip(paths, waves, es):
        e_o, valid = _oracle_emb(w, AO.resample(x, sr, 16000))                  # librosa.load(path, sr=16000), infer_v2_5.py:687
        alone = fe.emo_cond(p)
        assert e.shape == e_o.shape == alone.shape and e.dtype == alone.dtype
        assert float((e.cpu() - e_o)[0, valid].abs().max()) <= 1e-4 * float(e_o.abs().max())
        assert torch.equal(e[0, ~valid.to(DEV)], alone[0, ~valid.to(DEV)])        # the padded row: the engine's convention, batched or alone
