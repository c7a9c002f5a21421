"""Mixed-request batches on the real HIP engines (tiny random models): `IndexTTS2.infer_requests` runs requests of DIFFERENT voices with
their OWN sampling settings as one GPT batch / one codes -> mel call / one vocoder batch, and every request gets the audio it gets alone
(`infer_batch(voice, [text], ...)`); `codes_to_mel` with per-row speaker bundles equals the CPU oracle chain of every row under its own
bundle.  Design reference: per-request settings in one batch, backends/trt/serving/triton_server.py:96-305."""
import warnings

import numpy as np
import pytest
import torch

from tests.pipeline_stubs import StubFrontend
from tests.test_gpu_pipeline import _s2_engines, build

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


class VoiceFrontend(StubFrontend):
    """bundles that depend on the prompt's name: style, spk_cond_emb, and ref_mel / prompt_condition of different lengths; the stand-in
    codes -> mel reads the bundle too (a row rendered under another row's bundle would show in the waveform)"""

    def speaker_bundle(self, spk_audio_prompt):
        self.calls.append(("speaker", spk_audio_prompt))
        seed = sum(map(ord, str(spk_audio_prompt)))
        g = torch.Generator().manual_seed(seed)
        Tp = 4 + seed % 5
        return dict(style=(3.0 * torch.randn(1, 192, generator=g)).to(self.device), spk_cond_emb=torch.randn(1, 3 + seed % 4, 1024, generator=g).to(self.device),
                    ref_mel=torch.randn(1, self.n_mels, Tp, generator=g).to(self.device),
                    prompt_condition=torch.randn(1, Tp, 512, generator=g).to(self.device))

    def merge_emovec(self, spk_cond_emb, emo_cond_emb, alpha):          # the emotion vector is a function of the speaker's features, as in the model
        return ((self.emo.to(self.device) + spk_cond_emb.mean(dim=1)[:, : self.D]) * float(alpha))

    def codes_to_mel(self, codes, code_lens, bundle, duration_factor):
        mel, lens = super().codes_to_mel(codes, code_lens, bundle, duration_factor)
        off = float(bundle["style"].mean()) + 0.01 * bundle["ref_mel"].shape[-1]
        for b in range(mel.shape[0]):
            mel[b, :, : int(lens[b])] += off
        return mel, lens


REQUESTS = [
    dict(spk_audio_prompt="alice.wav", text="hello world", lang="en"),
    dict(spk_audio_prompt="bob.wav", text="hello world", lang="en"),
    dict(spk_audio_prompt="carol.wav", text="a much longer second sentence here. ok", lang="en"),
    dict(spk_audio_prompt="alice.wav", text="one more for the first voice", lang="en"),
    dict(spk_audio_prompt="bob.wav", text="and the last one", lang="en", emo_alpha=0.5, emo_audio_prompt="sad.wav"),
]


@pytest.fixture(scope="module")
def tts():
    t = build()
    t.frontend = VoiceFrontend(128, device=DEV)
    return t


def _alone(tts, req, **kw):
    r = dict(req)
    return tts.infer_batch(r.pop("spk_audio_prompt"), [r.pop("text")], r.pop("lang"), emo_audio_prompt=r.pop("emo_audio_prompt", None),
                           emo_alpha=r.pop("emo_alpha", 1.0), **r, **kw)[0]


def _check_equal(outs, refs, what):
    for i, ((sr, w), (sr0, w0)) in enumerate(zip(outs, refs)):
        assert sr == sr0 == 22050 and w.dtype == np.int16 and w.shape == w0.shape, f"{what}: request {i}: {w.shape} vs {w0.shape}"
        d = int(np.abs(w.astype(np.int32) - w0.astype(np.int32)).max())
        print(f"{what}: request {i}: {w.shape[0]} samples, max|d| vs the request alone {d}")
        assert d <= 1                                             # int16 rounding of identical floats (the bar of test_gpu_pipeline.py)
        assert np.abs(w0).max() > 0


def test_greedy_requests_equal_each_request_alone(tts):
    kw = dict(num_beams=1, top_k=1, max_mel_tokens=24)
    n_speaker = len([c for c in tts.frontend.calls if c[0] == "speaker"])
    outs = tts.infer_requests(REQUESTS, **kw)
    assert len([c for c in tts.frontend.calls if c[0] == "speaker"]) - n_speaker <= 3          # every distinct prompt is encoded once
    codes = tts.last_codes.cpu()
    assert not torch.equal(codes[0], codes[1]), "the same text under two voices must give different codes, or the test shows nothing"
    _check_equal(outs, [_alone(tts, r, **kw) for r in REQUESTS], "greedy")


def test_sampled_requests_with_their_own_settings_equal_each_request_alone(tts):
    own = [dict(temperature=0.7, top_p=0.9, seed=11), dict(temperature=1.2, top_p=0.6, seed=12), dict(temperature=1.0, top_p=1.0, seed=13, top_k=8),
           dict(temperature=0.9, top_p=0.8, seed=14, repetition_penalty=2.0), dict(temperature=1.1, top_p=0.7, seed=15, max_mel_tokens=9)]
    reqs = [dict(r, **o) for r, o in zip(REQUESTS, own)]
    kw = dict(num_beams=1, max_mel_tokens=24)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)          # (the capped request may run into its max_mel_tokens)
        outs = tts.infer_requests(reqs, **kw)
        refs = [_alone(tts, r, **{k: v for k, v in kw.items() if k not in r}) for r in reqs]
    _check_equal(outs, refs, "sampled")
    # and the settings matter: the first request under the second one's settings is another waveform
    other = tts.infer_requests([dict(reqs[0], **own[1])], **kw)[0][1]
    assert other.shape != outs[0][1].shape or np.abs(other.astype(np.int32) - outs[0][1].astype(np.int32)).max() > 1


def test_default_three_beam_mode_mixes_voices_but_not_settings(tts):
    outs = tts.infer_requests(REQUESTS[:3], max_mel_tokens=16)
    assert len(outs) == 3
    for sr, w in outs:
        assert sr == 22050 and w.dtype == np.int16 and w.shape[0] > 0 and np.abs(w).max() > 0
    with pytest.raises(ValueError, match="share"):
        tts.infer_requests([dict(REQUESTS[0], top_p=0.5), REQUESTS[1]], max_mel_tokens=16)


def test_codes_to_mel_with_per_row_bundles_vs_oracle_chain():
    """3 rows over 2 bundles (prompt lengths 11 and 7), code lengths 9 / 5 / 7, 4 steps, given noise: every row equals the CPU oracle chain of
    that row under ITS bundle, chained as test_v25_codes_to_mel_on_engine_vs_oracle_chain chains it, at that test's bar (2e-4)."""
    from indextts_amd.s2mel import codes_to_mel
    from oracle import codec_oracle as CO
    from oracle import s2mel_oracle as SO
    c, mm, (cc, rc, sc, csd, rsd, ssd, _) = _s2_engines("fp32")
    g = torch.Generator().manual_seed(60)
    bundles = []
    for Tp in (11, 7):
        bundles.append(dict(style=torch.randn(1, 192, generator=g).to(DEV), ref_mel=(torch.randn(1, 80, Tp, generator=g) * 0.5 - 1.0).to(DEV),
                            prompt_condition=torch.randn(1, Tp, 64, generator=g).to(DEV)))
    index = [0, 1, 0]
    lens = [9, 5, 7]
    codes = torch.randint(0, 8192, (3, 9), generator=g)
    target = [int(2 * n * 1.72) for n in lens]
    tp = [11, 7, 11]
    noise = torch.randn(3, 80, max(p + t for p, t in zip(tp, target)), generator=g)
    mel, mel_lens = codes_to_mel(c, mm.models, codes.to(DEV), torch.tensor(lens), bundles, 1.0, diffusion_steps=4, noise=noise.to(DEV),
                                 bundle_index=index)
    assert mel_lens.tolist() == target and mel.shape == (3, 80, max(target)) and bool(torch.isfinite(mel).all())
    for b, n in enumerate(lens):
        bd, Tp = bundles[index[b]], tp[b]
        T = Tp + target[b]
        with torch.no_grad():
            s = CO.codec_decode(csd, cc, codes[b:b + 1, :n])
            cond, _ = CO.length_regulator(rsd, rc, s, torch.tensor([target[b]]))
            cat = torch.cat([bd["prompt_condition"].cpu(), cond], 1)
            ref = SO.cfm_solve_euler(ssd, sc, noise[b:b + 1, :, :T], torch.tensor([T]), bd["ref_mel"].cpu(), cat, bd["style"].cpu(), 4, 0.7)
        err = float((mel[b:b + 1, :, : target[b]].cpu() - ref[:, :, Tp:]).abs().max())
        one, _ = codes_to_mel(c, mm.models, codes[b:b + 1, :n].to(DEV), torch.tensor([n]), bd, 1.0, diffusion_steps=4, noise=noise[b:b + 1, :, :T].to(DEV))
        own = float((mel[b:b + 1, :, : target[b]] - one).abs().max())
        print(f"per-row bundles, row {b} (bundle {index[b]}, Tp {Tp}): max|d| vs oracle chain {err:.2e}, vs the engine's single-bundle call {own:.2e}")
        assert err <= 2e-4


def test_ragged_prompt_padding_never_leaks():
    """`CFM.solve_euler` with per-row prompt lengths: what lies in a prompt tensor's padding (NaN here) must not reach the output, and a prompt
    tensor padded wider than the batch's frames must not raise."""
    _, mm, (_, _, sc, *_rest) = _s2_engines("fp32")
    cfm = mm.models["cfm"]
    g = torch.Generator().manual_seed(62)
    total, tp = [17, 13], [6, 3]
    T = max(total)
    mu = torch.randn(2, T, 64, generator=g)
    style = torch.randn(2, 192, generator=g)
    noise = torch.randn(2, 80, T, generator=g)
    prompt = torch.zeros(2, 80, T + 5)                            # wider than the frames of the batch
    for b in range(2):
        prompt[b, :, : tp[b]] = torch.randn(80, tp[b], generator=g) * 0.5 - 1.0
    clean = cfm.inference(mu.to(DEV), torch.tensor(total), prompt.to(DEV), style.to(DEV), None, 4, inference_cfg_rate=0.7, noise=noise.to(DEV),
                          prompt_lens=tp, frame_lens=total)
    dirty = prompt.clone()
    for b in range(2):
        dirty[b, :, tp[b]:] = float("nan")
    out = cfm.inference(mu.to(DEV), torch.tensor(total), dirty.to(DEV), style.to(DEV), None, 4, inference_cfg_rate=0.7, noise=noise.to(DEV),
                        prompt_lens=tp, frame_lens=total)
    for b in range(2):
        assert bool(torch.isfinite(out[b, :, : total[b]]).all())
        assert torch.equal(out[b, :, : total[b]], clean[b, :, : total[b]])
