"""Mixed-request batches in the reference's default 3-beam mode on the real HIP engines (tiny random models):
`IndexTTS2.infer_requests(beam_settings="own")` runs requests of DIFFERENT voices with their OWN sampling settings, caps, seeds as one beam
batch, and every request gets the audio it gets alone (`infer_batch(voice, [text], num_beams=3, seed=..., ...)`), whatever slot it lands in.
The default `beam_settings="shared"` keeps its refusal.  Design reference: per-request settings in one batch,
backends/trt/serving/triton_server.py:96-305; the default mode: indextts/infer_v2_5.py:732-740."""
import warnings

import numpy as np
import pytest
import torch

from tests.pipeline_stubs import StubFrontend
from tests.test_gpu_pipeline import build

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


class VoiceFrontend(StubFrontend):
    """bundles that depend on the prompt's name (as in tests/test_gpu_mixed_requests.py): style, spk_cond_emb, and ref_mel / prompt_condition
    of different lengths; the stand-in codes -> mel reads the bundle too (a row rendered under another row's bundle would show in the waveform)"""

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
OWN = [dict(temperature=0.7, top_p=0.9, seed=11), dict(temperature=1.2, top_p=0.6, seed=12), dict(temperature=1.0, top_p=1.0, seed=13, top_k=8),
       dict(temperature=0.9, top_p=0.8, seed=14, repetition_penalty=2.0), dict(temperature=1.1, top_p=0.7, seed=15, max_mel_tokens=9)]
KW = dict(num_beams=3, max_mel_tokens=24)


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
        assert d <= 1                                             # int16 rounding of identical floats (the bar of test_gpu_mixed_requests.py)
        assert np.abs(w0).max() > 0


@pytest.fixture(scope="module")
def alone(tts):
    """every request alone, through the scalar 3-beam path (computed once; shared, never modified)"""
    reqs = [dict(r, **o) for r, o in zip(REQUESTS, OWN)]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)          # (the capped request may run into its max_mel_tokens)
        return reqs, [_alone(tts, r, **{k: v for k, v in KW.items() if k not in r}) for r in reqs]


def test_beam_requests_with_their_own_settings_equal_each_request_alone(tts, alone):
    reqs, refs = alone
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        outs = tts.infer_requests(reqs, beam_settings="own", **KW)
    _check_equal(outs, refs, "3-beam, own settings")
    # and the settings matter: the first request under the second one's settings is another waveform
    other = tts.infer_requests([dict(reqs[0], **OWN[1])], beam_settings="own", **KW)[0][1]
    assert other.shape != outs[0][1].shape or np.abs(other.astype(np.int32) - outs[0][1].astype(np.int32)).max() > 1


def test_reversed_order_gives_the_same_waveforms(tts, alone):
    """slot independence: a request's draw is keyed by its seed and its segment index, not by the slot of its beam group"""
    reqs, refs = alone
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        outs = tts.infer_requests(reqs[::-1], beam_settings="own", **KW)
    _check_equal(outs[::-1], refs, "3-beam, own settings, reversed")


def test_shared_settings_still_refuse_differing_requests(tts, alone):
    reqs, _ = alone
    with pytest.raises(ValueError, match="share"):
        tts.infer_requests(reqs, beam_settings="shared", **KW)
    with pytest.raises(ValueError, match="share"):
        tts.infer_requests(reqs, **KW)                            # the default
