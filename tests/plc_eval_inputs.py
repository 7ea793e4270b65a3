"""Seeded inputs of the PLC evaluation fixtures G17 / G18, shared by tests/golden/make_golden_plc_stsim.py (which runs the
reference's PLC/PLC1_eval.py and PLC/PLC1_low_mid_high_eval.py on them) and the tests (which run the HIP path on the same
arrays)."""
import numpy as np

SR = 24000


def _pair(T, seed):
    """A tactile-like reference (a few partials with a slow envelope, plus noise) and a degraded estimate of it."""
    r = np.random.default_rng(seed)
    t = np.arange(T) / SR
    ref = np.zeros(T)
    for _ in range(4):
        f, ph, a = r.uniform(40.0, 900.0), r.uniform(0, 2 * np.pi), r.uniform(0.05, 0.3)
        ref += a * np.sin(2 * np.pi * f * t + ph) * (0.6 + 0.4 * np.sin(2 * np.pi * r.uniform(0.5, 3.0) * t))
    ref += 0.02 * r.standard_normal(T)
    est = 0.9 * ref + 0.03 * r.standard_normal(T) + 0.05 * np.sin(2 * np.pi * 1500.0 * t)
    return ref.astype(np.float32)[None], est.astype(np.float32)[None]


def _packets(T_lat, seed, packet=2, p=0.5):
    r = np.random.default_rng(seed)
    n = max(1, T_lat // packet)
    lost = np.repeat(r.random(n) < p, packet)[:T_lat]
    return np.concatenate([lost, np.zeros(T_lat - lost.size, bool)])


def _tokens(T_lat, idx):
    m = np.zeros(T_lat, bool)
    m[list(idx)] = True
    return m


# name -> (T_wave, T_lat, mask builder, signal seed).  T / T_lat = 320 gives 2 or 3 frames per token.
STSIM_CASES = {
    "frac":     (24077, 75, lambda L: _packets(L, 11), 101),        # T / T_lat not an integer
    "pk2":      (16000, 50, lambda L: _packets(L, 12), 102),        # packets of two, p = 0.5
    "odd":      (11890, 37, lambda L: _packets(L, 13), 103),        # odd T_lat (the last token is never lost)
    "all":      (9600, 30, lambda L: np.ones(L, bool), 104),        # all lost: unmasked subset empty
    "none":     (9600, 30, lambda L: np.zeros(L, bool), 105),       # none lost: masked subset empty
    "m3":       (8000, 25, lambda L: _tokens(L, [4]), 106),         # 3 masked frames (< 7: norm fall-through)
    "m6":       (8000, 25, lambda L: _tokens(L, [0, 2]), 107),      # 6 masked frames
    "m7":       (8000, 25, lambda L: _tokens(L, [1, 2, 3]), 108),   # 7 masked frames (the smallest SSIM subset)
    "u2":       (8000, 25, lambda L: ~_tokens(L, [10]), 109),       # 2 or 3 kept frames
    "tlat0":    (8000, 0, lambda L: np.zeros(0, bool), 110),        # T_lat = 0: (global, nan, nan)
}


def stsim_case(name):
    """-> ref [1, T], est [1, T] (float32), latent mask [T_lat] bool."""
    T, L, mk, seed = STSIM_CASES[name]
    ref, est = _pair(T, seed)
    return ref, est, mk(L)


# G18: two files at 24 kHz through pass 1 of eval_model: name -> (seconds, seed, tactile raw amplitude)
EVAL_FILES = {"f1": (1.0, 201, 0.37), "f2": (1.5, 202, 1.6)}
EVAL_MASK_SEED = 7000


def eval_file(name):
    """-> audio [1, T] and raw-amplitude tactile [1, T] at 24 kHz (float32), and the token mask [T // 320] the fixture fixes."""
    from multimodal_vqvae_compression_audio_tactile_amd import synth
    sec, seed, amp = EVAL_FILES[name]
    T = int(sec * SR)
    a = synth.audio_segments(1, seed=seed, T=T)[0].numpy()
    t = synth.tactile_segments(1, seed=seed, T=T)[0].numpy()
    t = (amp * t / max(float(np.abs(t).max()), 1e-8)).astype(np.float32)
    return a.astype(np.float32), t, _packets(T // 320, EVAL_MASK_SEED + seed)
