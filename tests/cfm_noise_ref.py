"""Host restatement of the engine's seeded flow-matching noise (include/indextts_hip.h, itts_s2mel_noise_forward): numpy, uint64 arithmetic,
evaluated in f64 and rounded once to f32.  The tests of the kernel and of every layer above it compare against this."""
import numpy as np

_TAG = np.uint64(0x43464D4E4F495345)
_G = np.uint64(0x9E3779B97F4A7C15)
_M1 = np.uint64(0xBF58476D1CE4E5B9)
_M2 = np.uint64(0x94D049BB133111EB)


def cfm_noise(seed: int, stream: int, n_frames: int, channels: int, temperature: float = 1.0, chunk: int = 0, first_frame: int = 0) -> np.ndarray:
    """(n_frames, channels) f32: the noise of target frames first_frame .. first_frame + n_frames - 1 (counted from the first frame after the prompt)."""
    with np.errstate(over="ignore"):
        a = np.uint64((int(stream) & 0xFFFFFFFF) | ((int(chunk) & 0xFFFFFFFF) << 32))
        j = np.arange(first_frame, first_frame + n_frames, dtype=np.uint64)[:, None]
        c = np.arange(channels, dtype=np.uint64)[None, :]
        b = j * np.uint64(channels) + c
        x = (np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF) ^ _TAG) + _G * (a + np.uint64(1)) + _M1 * (b + np.uint64(1))
        x = x ^ (x >> np.uint64(30))
        x = x * _M1
        x = x ^ (x >> np.uint64(27))
        x = x * _M2
        x = x ^ (x >> np.uint64(31))
    u1 = ((x >> np.uint64(32)).astype(np.float64) + 1.0) * 2.0 ** -32          # (0, 1]
    u2 = (x & np.uint64(0xFFFFFFFF)).astype(np.float64) * 2.0 ** -32           # [0, 1)
    z = np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2) * np.float64(np.float32(temperature))
    return z.astype(np.float32)


def cfm_noise_bct(seeds, streams, totals, prompt_lens, channels, temperatures=None, chunks=None) -> np.ndarray:
    """(B, channels, max total) f32 as `CFM.inference` lays noise out: row b holds zeros at its prompt frames and beyond its total, and its keyed
    noise at frames prompt_lens[b] .. totals[b] - 1."""
    B = len(seeds)
    out = np.zeros((B, channels, max(int(t) for t in totals)), dtype=np.float32)
    for b in range(B):
        n = int(totals[b]) - int(prompt_lens[b])
        if n > 0:
            z = cfm_noise(seeds[b], streams[b], n, channels, 1.0 if temperatures is None else temperatures[b], 0 if chunks is None else chunks[b])
            out[b, :, int(prompt_lens[b]):int(totals[b])] = z.T
    return out
