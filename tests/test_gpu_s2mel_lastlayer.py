"""GPU tests of the work the fp32x3 flow-matching solve no longer issues (engine options `s2mel_prune_last`, `x3_attn_skip`; both default on):

* `s2mel_prune_last`: with a tail layout (dead-row elimination, `CFM._tail_tables`) the LAST DiT layer's attention takes only the tail rows as
  queries and its wo / FFN norm / w1|w3 + SwiGLU / w2 stages run on the tail rows; the x_in GEMM reads its residual from `const_in` instead of
  accumulating into a per-step copy of it;
* `x3_attn_skip`: flash_attn_x3_kernel skips the fully masked half of a last key tile with at most 32 valid keys, and the MFMAs / softmax of a wave
  whose 32 queries are all past the sequence's end.

Nothing here has a tolerance: every skipped product is a product with an exact zero or belongs to a row nobody reads, so the results with an
option off and on must be the same BITS (`torch.equal`), in every combination, for ragged batches whose lengths hit the edges of the 64-key tile,
of the 256-query block and of the tail cut."""
import hashlib
import itertools

import pytest
import torch

from oracle import s2mel_oracle as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# sequence lengths: T % 64 covers {0, 1, 11, 32, 33, 63}; T % 256 leaves 2 (704: 192 queries, 447: 191), 1 (705: 193) and 7 (267, 288: 11 / 32
# queries) dead waves in the last query block of the full layout; the tails (T - cut) end in other places again
BATCHES = {
    # prompt lengths: a long one, none at all, one shorter than the halo (14 frames), a middling one
    "edges_a": ([704, 267, 289, 447], [140, 0, 9, 60]),
    "edges_b": ([705, 288], [200, 33]),
    # the second row's tail would be 16 frames = one WaveNet conv's padding: _tail_tables returns None, the solve runs without a tail layout
    "no_tail": ([391, 24], [140, 22]),
}
COMBOS = list(itertools.product((1, 0), (1, 0)))                  # (s2mel_prune_last, x3_attn_skip); the first one is the default


def _args_of(cfg):
    return dict(DiT=dict(hidden_dim=cfg.hidden_dim, num_heads=cfg.num_heads, depth=cfg.depth, in_channels=cfg.in_channels,
                         content_dim=cfg.content_dim, style_condition=True, final_layer_type="wavenet", is_causal=False,
                         long_skip_connection=True, uvit_skip_connection=True, time_as_token=False, style_as_token=False),
                wavenet=dict(hidden_dim=cfg.wavenet_hidden, num_layers=cfg.wavenet_layers, kernel_size=cfg.wavenet_kernel,
                             dilation_rate=cfg.wavenet_dilation_rate, style_condition=True),
                style_encoder=dict(dim=cfg.style_dim))


def _rms(a):
    return float(a.double().pow(2).mean().sqrt())


@pytest.fixture(scope="module")
def small_engine():
    """production widths (hidden 512, 8 heads, WaveNet 512), 3 DiT layers (one U-ViT skip), 3 WaveNet layers with a 14-frame halo"""
    from indextts_amd import s2mel
    cfg = S.S2MelConfig(depth=3, wavenet_layers=3, wavenet_dilation_rate=2)
    m = s2mel.CFM(_args_of(cfg), precision="fp32x3", device=DEV)
    m.load_state_dict(S.synth_weights(cfg, 5))
    return cfg, m


def _inputs(cfg, T, Tp, seed):
    g = torch.Generator().manual_seed(seed)
    B, Tm = len(T), max(T)
    x = torch.randn(B, 80, Tm, generator=g)
    mu = torch.randn(B, Tm, cfg.content_dim, generator=g)
    prompt = torch.randn(B, 80, max(max(Tp), 1), generator=g) * 0.5 - 1.0
    style = torch.randn(B, cfg.style_dim, generator=g)
    return x, mu, prompt, style


@pytest.mark.parametrize("cfg_rate", [0.7, 0.0])
@pytest.mark.parametrize("waves", [8, 4])
@pytest.mark.parametrize("batch", sorted(BATCHES))
def test_solve_is_bitwise_the_same_with_each_option_off(small_engine, batch, waves, cfg_rate):
    """3 Euler steps, CFG on (two branches) and off, the 8-wave and the 4-wave x3 GEMM (6 products): the mel with both options on equals the mel with
    either or both of them off, bit for bit, and a second solve with the defaults repeats it; and with a tail layout the pruned solve issues fewer GEMM FLOPs (the path under test is really taken)."""
    from indextts_amd import _lib
    cfg, m = small_engine
    T, Tp = BATCHES[batch]
    x, mu, prompt, style = _inputs(cfg, T, Tp, 6)
    t_span = torch.linspace(0, 1, 4)
    out, flops = {}, {}
    m.set_profiling(True)
    try:
        for prune, skip in COMBOS:
            with _lib.option_scope(x3_waves=waves, x3_products=6, s2mel_prune_last=prune, x3_attn_skip=skip):
                out[prune, skip] = m.solve_euler(x.clone(), torch.tensor(T), prompt, mu, style, None, t_span, cfg_rate, prompt_lens=Tp, frame_lens=T).cpu()
                flops[prune, skip] = m.profile()["gemm"]["flops"]
        # the default combination once more over a workspace of NaN patterns: the row-mapped wo epilogue (several sequences share an m-tile here) and the
        # tail-layout attention are stable run to run and read nothing they have not written
        m._ws.fill_(0xFF)
        with _lib.option_scope(x3_waves=waves, x3_products=6):
            again = m.solve_euler(x.clone(), torch.tensor(T), prompt, mu, style, None, t_span, cfg_rate, prompt_lens=Tp, frame_lens=T).cpu()
    finally:
        m.set_profiling(False)
    assert torch.equal(again, out[1, 1]), (batch, waves, cfg_rate, "second solve differs")
    ref = out[0, 0]
    assert _rms(ref) > 1e-3 and bool(torch.isfinite(ref).all())
    for k, y in out.items():
        assert torch.equal(y, ref), (batch, waves, cfg_rate, k, float((y - ref).abs().max()))
    print(f"{batch} waves={waves} cfg={cfg_rate}: 4 option combinations bitwise equal; GEMM FLOPs {flops[0, 0]:.4e} -> {flops[1, 1]:.4e}")
    if batch == "no_tail":
        assert flops[1, 1] == flops[0, 0]
    else:
        assert flops[1, 1] < flops[0, 0] and flops[1, 0] == flops[1, 1] and flops[0, 1] == flops[0, 0], flops


def test_solve_eight_products_and_f32_attention_unchanged(small_engine):
    """The variants beside the shipped one: 8 plane products (flash_attn_x3_kernel<8> takes the same tile modes), and x3_attn = 0 (the f32-MFMA flash
    kernel has no tail-layout form: the last layer keeps every row there, only the x_in GEMM's copy goes)."""
    from indextts_amd import _lib
    cfg, m = small_engine
    T, Tp = BATCHES["edges_a"]
    x, mu, prompt, style = _inputs(cfg, T, Tp, 8)
    t_span = torch.linspace(0, 1, 3)
    for extra in (dict(x3_products=8), dict(x3_attn=0)):
        out = {}
        for prune, skip in COMBOS:
            with _lib.option_scope(s2mel_prune_last=prune, x3_attn_skip=skip, **extra):
                out[prune, skip] = m.solve_euler(x.clone(), torch.tensor(T), prompt, mu, style, None, t_span, 0.7, prompt_lens=Tp, frame_lens=T).cpu()
        for k, y in out.items():
            assert _rms(y) > 1e-3 and torch.equal(y, out[0, 0]), (extra, k)


def test_single_estimator_call_unchanged(small_engine):
    """The estimator entry point has no tail layout: every row comes back, the same bits with the options on and off."""
    from indextts_amd import _lib
    cfg, m = small_engine
    T = [447, 267]
    g = torch.Generator().manual_seed(9)
    x = torch.randn(2, 80, max(T), generator=g)
    px = torch.randn(2, 80, max(T), generator=g) * 0.5
    mu = torch.randn(2, max(T), cfg.content_dim, generator=g)
    style = torch.randn(2, cfg.style_dim, generator=g)
    out = {}
    for prune, skip in COMBOS:
        with _lib.option_scope(s2mel_prune_last=prune, x3_attn_skip=skip):
            out[prune, skip] = m.estimator(x, px, torch.tensor(T), torch.full((2,), 0.3), style, mu, frame_lens=T).cpu()
    for k, y in out.items():
        assert _rms(y) > 1e-3 and torch.equal(y, out[0, 0]), k


def test_bench_geometry_bitwise_and_stable_run_to_run():
    """The production architecture (13 layers) on one utterance of 517 + 1926 frames with CFG (2 x 2443 rows: the last key tile holds 11 keys, the last
    query block 139 queries, the tail 1940 frames): two Euler steps, options off against on, and with the options on three solves on the same inputs
    over a workspace filled with NaN patterns return the same bits."""
    from indextts_amd import _lib, s2mel, synth
    args = synth.S2MEL_V2
    m = s2mel.CFM(args, precision="fp32x3", device=DEV)
    m.load_state_dict(synth.s2mel_weights(args, seed=1234))
    g = torch.Generator().manual_seed(0)
    Tp, T = 517, 517 + 1926
    x = torch.randn(1, 80, T, generator=g).to(DEV)
    mu = torch.randn(1, T, args["DiT"]["content_dim"], generator=g).to(DEV)
    prompt = (torch.randn(1, 80, Tp, generator=g) * 0.5 - 1.0).to(DEV)
    style = torch.randn(1, args["style_encoder"]["dim"], generator=g).to(DEV)
    t_span = torch.linspace(0, 1, 3)
    hsh = lambda y: hashlib.sha1(y.float().cpu().numpy().tobytes()).hexdigest()[:12]

    def solve():
        if m._ws is not None:
            m._ws.fill_(0xFF)
        return m.solve_euler(x.clone(), torch.tensor([T]), prompt, mu, style, None, t_span, 0.7, frame_lens=[T]).cpu()

    out = {}
    for prune, skip in COMBOS:
        with _lib.option_scope(s2mel_prune_last=prune, x3_attn_skip=skip):
            out[prune, skip] = solve()
    for k, y in out.items():
        assert bool(torch.isfinite(y).all()) and torch.equal(y, out[0, 0]), k
    bits = [hsh(solve()) for _ in range(3)]
    print(f"bench geometry: options off / on bitwise equal; three solves with the options on: {bits}")
    assert len(set(bits)) == 1 and bits[0] == hsh(out[1, 1])


def _attention(qkv, tab, frame, valid, heads, products, skip):
    from indextts_amd import _lib
    L = _lib.lib()
    H = heads * 64
    n_tok, t_max = sum(frame), max(frame)
    seq_T = torch.tensor(frame, dtype=torch.int32)
    seq_len = torch.tensor(valid, dtype=torch.int32)
    seq_start = torch.cumsum(seq_T, 0, dtype=torch.int32) - seq_T
    tok_seq = torch.repeat_interleave(torch.arange(len(frame), dtype=torch.int32), seq_T.long())
    tok_t = torch.arange(n_tok, dtype=torch.int32) - seq_start[tok_seq.long()]
    d = lambda t: t.to(DEV).contiguous()
    out = torch.full((n_tok, H), float("nan"), dtype=torch.float32, device=DEV)
    scratch = torch.empty(L.itts_s2mel_attention_scratch_bytes(n_tok, len(frame), heads, t_max, 2), dtype=torch.uint8, device=DEV)
    keep = [d(qkv), d(tab), d(tok_seq), d(tok_t), d(seq_start), d(seq_T), d(seq_len)]
    with _lib.option_scope(x3_products=products, x3_attn_skip=skip):
        _lib.check(L.itts_s2mel_attention_forward(*[_lib.ptr(t) for t in keep], len(frame), n_tok, t_max, heads, 2, _lib.ptr(out),
                                                  _lib.ptr(scratch), scratch.numel(), _lib.stream_ptr(torch.device(DEV))), "attention")
    return out.cpu()


@pytest.mark.parametrize("products", [6, 8])
def test_x3_attention_unit_skip_on_off(products):
    """itts_s2mel_attention_forward (fp32x3) on the same set of lengths, plus rows whose valid key count is shorter than their frames (11 and 33 valid
    keys: one masked half-tile skipped, one kept), a 5-frame sequence and a whole number of tiles and blocks (512): x3_attn_skip = 1 gives the bits of 0,
    every row is written, and the result is the f64 attention's within the x3 kernel's usual 2e-5."""
    frame = [704, 705, 267, 288, 289, 447, 5, 512]
    valid = [704, 700, 11, 32, 33, 447, 5, 512]
    heads = 2
    H = heads * 64
    g = torch.Generator().manual_seed(3)
    qkv = torch.randn(sum(frame), 3 * H, generator=g)
    qkv[:, 2 * H:] *= torch.exp(torch.randn(1, H, generator=g))      # wide dynamic range over the value channels
    tab = S.rope_table(S.S2MelConfig(hidden_dim=H, num_heads=heads), max(frame))
    off = _attention(qkv, tab, frame, valid, heads, products, 0)
    on = _attention(qkv, tab, frame, valid, heads, products, 1)
    assert bool(torch.isfinite(off).all()) and bool(torch.isfinite(on).all())
    assert torch.equal(on, off), float((on - off).abs().max())
    ref = torch.zeros(sum(frame), H, dtype=torch.float64)
    o = 0
    for T, n in zip(frame, valid):
        q, k, v = qkv[o:o + T].double().split(H, dim=-1)
        q = S.apply_rope(q.view(1, T, heads, 64), tab[:T].double()).transpose(1, 2)
        k = S.apply_rope(k.view(1, T, heads, 64), tab[:T].double()).transpose(1, 2)
        v = v.view(1, T, heads, 64).transpose(1, 2)
        sc = (q @ k.transpose(-1, -2)) / 8.0
        sc[..., n:] = float("-inf")
        ref[o:o + T] = (torch.softmax(sc, -1) @ v).transpose(1, 2).reshape(T, H)
        o += T
    err = float((on.double() - ref).abs().max())
    print(f"x3 attention unit ({products} products): skip on == off bitwise; max|d| vs f64 = {err:.3e}")
    assert err < 2e-5
