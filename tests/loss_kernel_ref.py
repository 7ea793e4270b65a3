"""Float64 restatements of the loss kernels' contracts (csrc/kernels_loss.hip), one function per kernel -- test
infrastructure, no test in here.  Each is written from the kernel's header comment and the reference's formula
(Training/compare_dacvsproposal_5.py:150-211), in plain torch / numpy on the CPU.  Layout as on the device: a plane is
[rows, B*nfr] with column b*nfr + n; here the column axis is kept as [B, nfr] where that reads better.

``mrstft_chain`` / ``melcos_chain`` / ``l1_chain`` compose them into the loss value and d loss / d y the way losses.py does;
tests/test_loss_kernel_ref_cpu.py holds those against autograd on oracle/losses_torch.py, so that a misconception shared by a
kernel and its restatement cannot hide.
"""
import math

import numpy as np
import torch

U = 2.0 ** -24                     # unit roundoff of fp32
F64 = torch.float64


def f32(v):
    """The value a C float argument takes (eps, coef), as a Python float."""
    return float(np.float32(v))


def sanitize(x):
    return torch.nan_to_num(x, nan=0.0, posinf=0.0, neginf=0.0)


def hann(n_fft):
    return torch.hann_window(n_fft, periodic=True, dtype=F64)


def dft_basis(n_fft):
    """[2F, n_fft]: rows 0..F-1 = cos(2 pi k f / n), rows F..2F-1 = -sin(...), F = n_fft/2 + 1."""
    F = n_fft // 2 + 1
    k = torch.arange(F, dtype=F64).unsqueeze(1)
    f = torch.arange(n_fft, dtype=F64).unsqueeze(0)
    ang = 2.0 * math.pi * ((k * f) % n_fft) / n_fft
    return torch.cat([torch.cos(ang), -torch.sin(ang)], 0)


def padded_basis(n_fft):
    """The basis as the device holds it: [2Fp, n_fft] with Fp = F rounded up to 32, zero rows as padding."""
    F = n_fft // 2 + 1
    Fp = (F + 31) // 32 * 32
    W = torch.zeros(2 * Fp, n_fft, dtype=F64)
    Wd = dft_basis(n_fft)
    W[:F] = Wd[:F]; W[Fp:Fp + F] = Wd[F:]
    return W, F, Fp


def nframes(T, hop):
    return 1 + T // hop


def frame_index(T, n_fft, hop):
    """[n_fft, nfr] sample index that frame n, tap f reads: torch 'reflect' padding of n_fft/2 on both sides."""
    nfr = nframes(T, hop)
    j = torch.arange(nfr).unsqueeze(0) * hop + torch.arange(n_fft).unsqueeze(1) - n_fft // 2
    j = j.abs()
    return torch.where(j >= T, 2 * (T - 1) - j, j)


def stft_frames(x, window, n_fft, hop):
    """x[B, T] -> [n_fft, B, nfr] = window[f] * finite_or_zero(x)[b, reflect(n*hop + f - n_fft/2)]."""
    idx = frame_index(x.shape[1], n_fft, hop)
    xs = sanitize(x.to(F64))
    return window.to(F64).reshape(-1, 1, 1) * xs[:, idx].permute(1, 0, 2)


def spec_mag(re, im, eps):
    return (re.to(F64) ** 2 + im.to(F64) ** 2).sqrt().clamp_min(eps)


def spec_loss_sums(X, Y):
    """X, Y [F, B, nfr] -> [3, B]: sum (X-Y)^2, sum Y^2, sum |X-Y| per item."""
    X, Y = X.to(F64), Y.to(F64)
    d = X - Y
    return torch.stack([(d * d).sum(dim=(0, 2)), (Y * Y).sum(dim=(0, 2)), d.abs().sum(dim=(0, 2))])


def spec_grad(re, im, X, Y, coef_a, coef_b, extra, eps):
    """All [F, B, nfr] (coef_a [B] or None, extra or None): gX = coef_a[b]*(X-Y) + coef_b*sign(X-Y) + extra, then through
    |z| clamped at eps: z/|z| where |z| >= eps (and |z| > 0), 0 below.  -> (gre, gim, gX)."""
    re, im, X, Y = (t.to(F64) for t in (re, im, X, Y))
    d = X - Y
    gX = coef_b * torch.sign(d)
    if coef_a is not None:
        gX = gX + coef_a.to(F64).reshape(1, -1, 1) * d
    if extra is not None:
        gX = gX + extra.to(F64)
    a = (re * re + im * im).sqrt()
    live = (a >= eps) & (a > 0)
    safe = torch.where(live, a, torch.ones_like(a))
    zero = torch.zeros_like(a)
    return torch.where(live, gX * re / safe, zero), torch.where(live, gX * im / safe, zero), gX


def overlap_add(dF, window, T, hop, dy0=None):
    """The adjoint of framing: dy[b, reflect(n*hop + f - n_fft/2)] += window[f] * dF[f, b, n].  dF [n_fft, B, nfr]."""
    n_fft, B, nfr = dF.shape
    idx = frame_index(T, n_fft, hop)                                     # [n_fft, nfr]
    contrib = (window.to(F64).reshape(-1, 1, 1) * dF.to(F64)).permute(1, 0, 2).reshape(B, -1)
    dy = torch.zeros(B, T, dtype=F64) if dy0 is None else dy0.to(F64).clone()
    dy.scatter_add_(1, idx.reshape(1, -1).expand(B, -1), contrib)
    return dy


def l1_loss(y, tgt):
    """-> (sum |d|, sign(d)) with d = finite_or_zero(y) - finite_or_zero(tgt)."""
    d = sanitize(y.to(F64)) - sanitize(tgt.to(F64))
    return d.abs().sum(), torch.sign(d)


def mel_max(M):
    """M [n_mels, B, nfr] -> (max [B], argmax [B]): the first maximum in row-major (mel, frame) order."""
    flat = M.permute(1, 0, 2).reshape(M.shape[1], -1).numpy()
    arg = flat.argmax(axis=1)                                            # numpy: first occurrence
    return torch.from_numpy(flat[np.arange(flat.shape[0]), arg].copy()), torch.from_numpy(arg.astype(np.int64))


def mel_cos(Mx, My, maxx, maxy, eps, use_log=True, coef=None, clamp_grad=True):
    """Mx, My [n_mels, B, nfr], maxx, maxy [B] -> cos [B, nfr] = clamp(<X,Y> / max(|X||Y|, eps), -1, 1) with
    X = log(Mx/max(maxx, eps) + eps) (use_log) or Mx/max(maxx, eps).  With coef (= dL/dcos of every column) also
    dM = dL/dMx and dden [B, nfr] = each column's share of dL/d(denx), by autograd with the maximum held constant.
    clamp_grad=False lets the gradient through the clamp(-1, 1) whatever v is (the 'inside' branch, for columns at the gate)."""
    B, nfr = Mx.shape[1], Mx.shape[2]
    Mx = Mx.to(F64).clone().requires_grad_(coef is not None)
    My = My.to(F64)
    denx = maxx.to(F64).clamp_min(eps).reshape(B, 1).expand(B, nfr).clone().requires_grad_(coef is not None)
    deny = maxy.to(F64).clamp_min(eps).reshape(B, 1)
    X, Y = Mx / denx, My / deny
    if use_log:
        X, Y = (X + eps).log(), (Y + eps).log()
    num = (X * Y).sum(0)
    prod = torch.linalg.vector_norm(X, dim=0) * torch.linalg.vector_norm(Y, dim=0)
    v = num / prod.clamp_min(eps)
    cosv = v.clamp(-1.0, 1.0)
    if coef is None:
        return cosv.detach(), None, None
    dM, dden = torch.autograd.grad(coef * (cosv if clamp_grad else v).sum(), (Mx, denx))
    return cosv.detach(), dM, dden


def mel_max_grad(dM, dden, maxv, argm, eps):
    """dM [n_mels, B, nfr], dden [B, nfr]: item b's argmax element gains sum_n dden[b, n] where maxv[b] >= eps."""
    out = dM.to(F64).clone()
    nfr = dM.shape[2]
    g = dden.to(F64).sum(1)
    for b in range(dM.shape[1]):
        if float(maxv[b]) >= eps:
            e = int(argm[b])
            out[e // nfr, b, e % nfr] += g[b]
    return out


# ---- the kernels' contracts chained the way losses.py chains the kernels (float64 throughout) ---------------------------
def _spectrum(x, n_fft, hop, eps):
    W = dft_basis(n_fft)
    F = n_fft // 2 + 1
    fr = stft_frames(x, hann(n_fft), n_fft, hop)                         # [n_fft, B, nfr]
    S = torch.einsum("kf,fbn->kbn", W, fr)
    return S[:F], S[F:], spec_mag(S[:F], S[F:], eps)


def _spectrum_backward(gre, gim, n_fft, hop, T):
    W = dft_basis(n_fft)
    dF = torch.einsum("kf,kbn->fbn", W, torch.cat([gre, gim], 0))
    return overlap_add(dF, hann(n_fft), T, hop)


def l1_chain(y, tgt):
    """y, tgt [B, T] -> (mean |d|, d/dy)."""
    s, sg = l1_loss(y, tgt)
    return s / y.numel(), sg / y.numel()


def mrstft_chain(y, tgt, ffts=(256, 512, 1024), hops=(64, 128, 256), eps=1e-7):
    """y, tgt [B, T] float64 -> (MultiResSTFTLoss value, d value / d y)."""
    B, T = y.shape
    res = [(n, h) for n, h in zip(ffts, hops) if T >= max(8, n // 2)]
    if not res:
        v, g = l1_chain(y, tgt)
        return 0.1 * v, 0.1 * g
    value, dy = 0.0, torch.zeros(B, T, dtype=F64)
    for n_fft, hop in res:
        F = n_fft // 2 + 1
        re, im, X = _spectrum(y, n_fft, hop, eps)
        _, _, Y = _spectrum(tgt, n_fft, hop, eps)
        nfr = X.shape[2]
        s = spec_loss_sums(X, Y)
        num, den = s[0].sqrt(), s[1].sqrt().clamp_min(eps)
        value = value + 0.5 * ((num / den).mean() + s[2].sum() / (B * F * nfr)) / len(res)
        coef_a = torch.where(num > 0, 1.0 / (B * num * den), torch.zeros_like(num)) * (0.5 / len(res))
        gre, gim, _ = spec_grad(re, im, X, Y, coef_a, 0.5 / len(res) / (B * F * nfr), None, eps)
        dy += _spectrum_backward(gre, gim, n_fft, hop, T)
    return value, dy


def melcos_chain(y, tgt, fb, n_fft=512, hop=128, eps=1e-7):
    """y, tgt [B, T] float64, fb [F, n_mels] -> (MelCosineLoss value, d value / d y)."""
    B, T = y.shape
    fb = fb.to(F64)
    re, im, X = _spectrum(y, n_fft, hop, eps)
    _, _, Y = _spectrum(tgt, n_fft, hop, eps)
    Mx, My = torch.einsum("km,kbn->mbn", fb, X), torch.einsum("km,kbn->mbn", fb, Y)
    nfr = X.shape[2]
    maxx, argx = mel_max(Mx)
    maxy, _ = mel_max(My)
    cosv, dM, dden = mel_cos(Mx, My, maxx, maxy, eps, True, coef=-1.0 / (B * nfr))
    dM = mel_max_grad(dM, dden, maxx, argx, eps)
    extra = torch.einsum("km,mbn->kbn", fb, dM)
    gre, gim, _ = spec_grad(re, im, X, Y, None, 0.0, extra, eps)
    return 1.0 - cosv.sum() / (B * nfr), _spectrum_backward(gre, gim, n_fft, hop, T)
