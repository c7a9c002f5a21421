"""`cfm_noise="request"` through the pipeline on the real HIP engines (tiny random models, the engine's codec and s2mel stages -- not a stand-in
codes -> mel): a request's AUDIO is the audio it gets alone, in any batch and any order; the same call twice is the same audio without
`torch.manual_seed`; a stream run twice with one seed yields equal chunks; and the default is still torch's generator."""
import numpy as np
import pytest
import torch

from tests.pipeline_stubs import StubFrontend
from tests.test_gpu_pipeline import _s2_engines, build

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


class VoiceFrontend(StubFrontend):
    """bundles that depend on the prompt's name, shaped for the tiny s2mel engines: style, spk_cond_emb, and ref_mel (80 bands) / prompt_condition
    (64 wide) of different lengths"""

    def speaker_bundle(self, spk_audio_prompt):
        self.calls.append(("speaker", spk_audio_prompt))
        seed = sum(map(ord, str(spk_audio_prompt)))
        g = torch.Generator().manual_seed(seed)
        Tp = 4 + seed % 5
        return dict(style=torch.randn(1, 192, generator=g).to(self.device), spk_cond_emb=torch.randn(1, 3 + seed % 4, 1024, generator=g).to(self.device),
                    ref_mel=(torch.randn(1, 80, Tp, generator=g) * 0.5 - 1.0).to(self.device),
                    prompt_condition=torch.randn(1, Tp, 64, generator=g).to(self.device))

    def merge_emovec(self, spk_cond_emb, emo_cond_emb, alpha):
        return ((self.emo.to(self.device) + spk_cond_emb.mean(dim=1)[:, : self.D]) * float(alpha))

    def codes_to_mel(self, codes, code_lens, bundle, duration_factor):
        raise AssertionError("the engine's codes -> mel stages must run, not the frontend's")


REQUESTS = [
    dict(spk_audio_prompt="alice.wav", text="hello world", lang="en", seed=11),
    dict(spk_audio_prompt="bob.wav", text="hello world", lang="en", seed=12),
    dict(spk_audio_prompt="carol.wav", text="a much longer second sentence here. ok", lang="en", seed=13),
    dict(spk_audio_prompt="alice.wav", text="one more for the first voice", lang="en", seed=14),
    dict(spk_audio_prompt="bob.wav", text="and the last one", lang="en", seed=15),
]
KW = dict(num_beams=1, max_mel_tokens=24, cfm_noise="request")


@pytest.fixture(scope="module")
def tts():
    t = build()
    t.frontend = VoiceFrontend(128, device=DEV)
    t.semantic_codec, t.s2mel = _s2_engines("fp32")[:2]
    return t


@pytest.fixture(scope="module")
def alone(tts):
    """every request alone through infer_batch, once"""
    out = []
    for req in REQUESTS:
        r = dict(req)
        out.append(tts.infer_batch(r.pop("spk_audio_prompt"), [r.pop("text")], r.pop("lang"), **r, **KW)[0])
    return out


def _check_equal(outs, refs, what):
    for i, ((sr, w), (sr0, w0)) in enumerate(zip(outs, refs)):
        assert sr == sr0 == 22050 and w.dtype == np.int16 and w.shape == w0.shape, f"{what}: request {i}: {w.shape} vs {w0.shape}"
        d = int(np.abs(w.astype(np.int32) - w0.astype(np.int32)).max())
        print(f"{what}: request {i}: {w.shape[0]} samples, max|d| vs the request alone {d}")
        assert d <= 1                                             # the bar of tests/test_gpu_mixed_requests.py
        assert np.abs(w0).max() > 0


def test_requests_get_the_audio_they_get_alone_in_any_order(tts, alone):
    torch.manual_seed(1)
    outs = tts.infer_requests(REQUESTS, **KW)
    _check_equal(outs, alone, "mixed batch")
    torch.manual_seed(2)                                          # whatever torch's generator holds
    rev = tts.infer_requests(REQUESTS[::-1], **KW)[::-1]
    _check_equal(rev, alone, "reversed batch")


def test_same_call_twice_is_the_same_audio_and_the_seed_matters(tts):
    a = tts.infer_batch("alice.wav", ["hello world"], "en", seed=5, **KW)[0][1]
    torch.randn(7, device=DEV)                                    # draws in between change nothing
    b = tts.infer_batch("alice.wav", ["hello world"], "en", seed=5, **KW)[0][1]
    assert np.array_equal(a, b)
    c = tts.infer_batch("alice.wav", ["hello world"], "en", seed=6, **KW)[0][1]
    assert c.shape != a.shape or np.abs(c.astype(np.int32) - a.astype(np.int32)).max() > 1
    # greedy codes (top_k = 1): the codes do not depend on the seed, so the difference is the flow-matching noise alone
    g5 = tts.infer_batch("alice.wav", ["hello world"], "en", seed=5, top_k=1, **KW)[0][1]
    g6 = tts.infer_batch("alice.wav", ["hello world"], "en", seed=6, top_k=1, **KW)[0][1]
    assert g5.shape == g6.shape and np.abs(g5.astype(np.int32) - g6.astype(np.int32)).max() > 1


def test_stream_twice_with_one_seed_yields_equal_chunks(tts):
    texts = ["a first streamed sentence", "short"]
    kw = dict(max_mel_tokens=24, chunk_size=8, overlap_size=2, seed=9, cfm_noise="request")
    runs = []
    for _ in range(2):
        torch.randn(3, device=DEV)
        runs.append([(audio, list(done)) for _, audio, done in tts.infer_stream("spk.wav", texts, "en", **kw)])
    assert len(runs[0]) == len(runs[1]) >= 2
    n_audio = 0
    for (a0, d0), (a1, d1) in zip(*runs):
        assert d0 == d1
        for x, y in zip(a0, a1):
            assert (x is None) == (y is None)
            if x is not None:
                n_audio += 1
                assert np.array_equal(x, y)
    assert n_audio >= 3


def test_default_mode_still_draws_from_torch_generator(tts):
    kw = dict(num_beams=1, max_mel_tokens=24, seed=5)
    torch.manual_seed(0)
    a = tts.infer_batch("alice.wav", ["hello world"], "en", **kw)[0][1]
    torch.manual_seed(0)
    state = torch.cuda.get_rng_state(0).clone()
    b = tts.infer_batch("alice.wav", ["hello world"], "en", **kw)[0][1]
    assert np.array_equal(a, b)
    assert not torch.equal(torch.cuda.get_rng_state(0), state)    # the noise came from the device generator
    c = tts.infer_batch("alice.wav", ["hello world"], "en", **kw)[0][1]          # ... so without re-seeding the audio differs
    assert c.shape == a.shape and np.abs(c.astype(np.int32) - a.astype(np.int32)).max() > 1


def test_v2_codes_latent_to_mel_keyed_is_the_given_noise_path():
    """The IndexTTS-2 (v2) codes + latent -> mel stage with `noise_keys`: 3 rows (code lengths 9 / 5 / 7, prompt 11 frames), per-row noise
    temperatures; equal to the same call given the kernel's rows as `noise=`, torch's generator untouched, and every row equal to the row alone
    (printed; the 2e-4 of the codes -> mel oracle tests)."""
    from indextts_amd.infer_v2 import IndexTTS2 as IndexTTS2V2
    from tests.test_gpu_pipeline import _bundle_for_s2
    c, mm, _ = _s2_engines("fp32", gpt_latent=True, gpt_dim=128)
    v2 = object.__new__(IndexTTS2V2)                              # the stage reads the two engine stages only
    v2.semantic_codec, v2.s2mel, v2.frontend = c, mm, None
    cfm = mm.models["cfm"]
    bundle = _bundle_for_s2(StubFrontend(128, device=DEV))
    g = torch.Generator().manual_seed(77)
    lens, Tp = [9, 5, 7], 11
    codes = torch.randint(0, 8192, (3, 9), generator=g).to(DEV)
    latent = (torch.randn(3, 9, 128, generator=g) * 0.3).to(DEV)
    target = [int(n * 1.72) for n in lens]
    total = [Tp + t for t in target]
    seeds, streams, temps = [31, 32, 31], [0, 0, 1], [1.0, 0.8, 1.0]
    state = torch.cuda.get_rng_state(0).clone()
    mel, mel_lens = v2.codes_latent_to_mel(codes, torch.tensor(lens), latent, bundle, diffusion_steps=4, noise_keys=(seeds, streams),
                                           noise_temperature=temps)
    assert torch.equal(torch.cuda.get_rng_state(0), state)
    assert mel_lens.tolist() == target and mel.shape == (3, 80, max(target)) and bool(torch.isfinite(mel).all())
    tabs, n_tok, _ = cfm._tables(total, torch.tensor(total), 1)
    rows = cfm.noise_rows(tabs["tok_seq"], tabs["tok_t"], [Tp] * 3, seeds, streams, temps, n_tok)
    noise = cfm._unpack_rows(rows, tabs["tok_seq"].long(), tabs["tok_t"].long(), 3, max(total))
    given, _ = v2.codes_latent_to_mel(codes, torch.tensor(lens), latent, bundle, diffusion_steps=4, noise=noise)
    assert torch.equal(mel, given)
    for b, n in enumerate(lens):
        one, _ = v2.codes_latent_to_mel(codes[b:b + 1, :n], torch.tensor([n]), latent[b:b + 1, :n], bundle, diffusion_steps=4,
                                        noise_keys=([seeds[b]], [streams[b]]), noise_temperature=temps[b])
        own = float((mel[b:b + 1, :, : target[b]] - one).abs().max())
        print(f"v2 codes + latent -> mel, keyed, row {b}: max|d| vs the row alone {own:.2e}")
        assert own <= 2e-4
    other, _ = v2.codes_latent_to_mel(codes, torch.tensor(lens), latent, bundle, diffusion_steps=4, noise_keys=([41, 42, 41], streams),
                                      noise_temperature=temps)
    assert float((other - mel).abs().max()) > 1e-3                # the seed matters
