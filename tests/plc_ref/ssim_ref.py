"""Restatement of the ST-SIM core of PLC/PLC1_eval.py:_stsim_core for the tests and the G17 generator.

``structural_similarity`` restates skimage.metrics.structural_similarity(im1, im2, data_range=1.0) with its defaults for 2-D
images (scikit-image is not a dependency): win_size 7, uniform window scipy.ndimage.uniform_filter(size=7, mode='reflect'),
use_sample_covariance (cov_norm = 49/48), K1 = 0.01, K2 = 0.03, the map cropped by 3 on every side, mean in float64; an
image side < 7 raises ValueError as skimage does.  ``dtype=np.float32`` keeps float32 inputs in float32 as skimage does;
float64 is the exact-value yardstick.  ``norm_sim`` is the reference's fallback formula, ``stsim_with_mask`` the host glue of
compute_stsim_mel_with_mask (float64 frame -> token rule, concatenated subset columns, the ValueError fall-through)."""
import numpy as np
from scipy.ndimage import uniform_filter

WIN = 7
HOP = 128


def structural_similarity(im1, im2, data_range=1.0, dtype=np.float64):
    im1, im2 = np.asarray(im1), np.asarray(im2)
    if im1.shape != im2.shape:
        raise ValueError("Input images must have the same dimensions.")
    if np.any(np.asarray(im1.shape) - WIN < 0):
        raise ValueError("win_size exceeds image extent.")
    a, b = im1.astype(dtype), im2.astype(dtype)
    cov_norm = dtype(WIN * WIN) / dtype(WIN * WIN - 1)
    f = lambda x: uniform_filter(x, size=WIN)
    ux, uy = f(a), f(b)
    uxx, uyy, uxy = f(a * a), f(b * b), f(a * b)
    vx = cov_norm * (uxx - ux * ux)
    vy = cov_norm * (uyy - uy * uy)
    vxy = cov_norm * (uxy - ux * uy)
    C1, C2 = dtype((0.01 * data_range) ** 2), dtype((0.03 * data_range) ** 2)
    A1, A2 = 2 * ux * uy + C1, 2 * vxy + C2
    B1, B2 = ux ** 2 + uy ** 2 + C1, vx + vy + C2
    S = (A1 * A2) / (B1 * B2)
    p = (WIN - 1) // 2
    return float(S[p:-p, p:-p].mean(dtype=np.float64))


def ssim_f32(im1, im2, data_range=1.0):
    return structural_similarity(im1, im2, data_range, dtype=np.float32)


def norm_sim(A, B):
    """max(0, 1 - |A-B| / (|A| + |B| + 1e-12)) in float64."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    return float(max(0.0, 1.0 - np.linalg.norm(A - B) / (np.linalg.norm(A) + np.linalg.norm(B) + 1e-12)))


def stsim_core(A, B, backend="ssim", ssim=structural_similarity):
    if backend == "ssim":
        try:
            return float(ssim(A, B, data_range=1.0))
        except ValueError:
            pass
    return norm_sim(A, B)


def frame_mask(latent_mask, T_wave, n_frames):
    lm = np.asarray(latent_mask, bool).reshape(-1)
    if lm.size == 0 or T_wave == 0 or n_frames == 0:
        return np.zeros(n_frames, bool)
    spt = float(T_wave) / float(lm.size)
    tok = np.clip(np.floor((np.arange(n_frames) * HOP) / spt).astype(np.int64), 0, lm.size - 1)
    return lm[tok]


def stsim_with_mask(X, Y, latent_mask, T_wave, backend="ssim", ssim=structural_similarity):
    """(global, masked, unmasked) of normalised mel images X, Y [64, T_f]."""
    g = stsim_core(X, Y, backend, ssim)
    lm = np.asarray(latent_mask, bool).reshape(-1)
    if lm.size == 0 or T_wave == 0 or X.shape[1] == 0:
        return g, float("nan"), float("nan")
    fm = frame_mask(lm, T_wave, X.shape[1])
    sub = lambda m: float("nan") if not m.any() else stsim_core(X[:, m], Y[:, m], backend, ssim)
    return g, sub(fm), sub(~fm)
