"""-m gpu: every loss kernel (csrc/kernels_loss.hip, row f2) on its own against its float64 restatement
(tests/loss_kernel_ref.py, held to the oracle by tests/test_loss_kernel_ref_cpu.py) on identical fp32 inputs.

Inputs are synthesised in fp32 on the CPU from a seeded generator and the same bits go to the device; no kernel's output is
fed to the next.  Where a kernel is one rounding of an exact float64 expression (stft_frames, the l1 gradient, mel_max) the
comparison is bit-for-bit.  Elsewhere the bound is  |got - want| <= k * u * scale,  u = 2^-24:  scale is the float64 sum of
the absolute values of the terms the kernel adds (the value itself for a product, a square root or a sum of non-negative
terms), k the count of fp32 roundings on the kernel's longest path, read off the source (the library is built with
-ffp-contract=off: no fused multiply-add changes the count); device sqrtf and logf are allowed 2 ulp = 4u each.

    kernel            k, as asserted                                                              largest error/(u*scale) seen
    DFT GEMM          n_fft (any-order summation of n_fft products)                               4.76
    spec_mag          6 = re*re|im*im, +, sqrt (4)                                                1.75
    spec_loss_sums    3 (d, d*d: twice d's rounding and its own) + ceil(F*nfr/4096) serial adds
                      + 8 tree levels + rowsum (1 + 8)                                            2.07
    spec_grad         12 = gX (d, coef_a*d, two adds) 4 + |z| as in spec_mag 6 + gX*re, /|z| 2       4.81
    overlap_add       3*n_fft/hop + 2                                                             2.49
    l1_loss_sum       1 (d) + ceil(n/(256*P)) serial + 8 tree + rowsum (ceil(P/256) + 8)          1.84
    mel_cos           first-order propagation of each operation's rounding through the formula
                      (_mel_cos_bounds: per element u*(2 + 4|X|) on X = log(M/den + eps), 65u per
                      64-term dot product, ...), i.e. k*u*scale term by term                      cos 0.065, dM 0.068, dden 0.017
    mel_max_grad_     ceil(nfr/256) serial + 8 tree + 1 (the add into dM)                         0.25

An element whose float64 value lies within its bound of a gate (|z| against eps, v against +-1) may take either branch; at
most 1 % of a case's elements may be excused so, and the planted gate elements (|z| == eps exactly, ...) are never excused.
"""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import loss_kernel_ref as R                      # noqa: E402

pytestmark = pytest.mark.gpu

U = R.U
F64 = torch.float64
SHAPES = [(256, 64, 1, 129), (256, 64, 3, 191), (256, 64, 3, 192), (256, 64, 3, 193), (512, 128, 2, 257),
          (1024, 256, 2, 513), (1024, 256, 2, 700), (256, 64, 2, 1000), (256, 64, 3, 5600)]
NONFINITE = (float("nan"), float("inf"), float("-inf"))


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float32)


def _rand(g, *shape):
    return torch.rand(*shape, generator=g, dtype=torch.float32)


def _bits_equal(got, want32):
    return torch.equal(got.cpu().contiguous().view(torch.int32), want32.contiguous().view(torch.int32))


def _ratio(name, got, want, bound_over_k, k, excused=None, err=None):
    """Largest |got - want| / (u * scale); asserts it is within k.  bound_over_k = u * scale per element (float64)."""
    if err is None:
        err = (got.detach().cpu().to(F64) - want).abs()
    exact = bound_over_k == 0
    assert bool((err[exact] == 0).all()), f"{name}: an element with zero scale differs"
    r = torch.where(exact, torch.zeros_like(err), err / torch.where(exact, torch.ones_like(err), bound_over_k))
    if excused is not None:
        assert int(excused.sum()) <= 0.01 * excused.numel(), f"{name}: {int(excused.sum())} of {excused.numel()} elements at a gate"
        r = torch.where(excused, torch.zeros_like(r), r)
    worst = float(r.max()) if r.numel() else 0.0
    print(f"{name}: largest error/(u*scale) {worst:.3f} against k = {k}")
    assert worst <= k, f"{name}: error {worst:.3f} u*scale exceeds the derived k = {k}"
    return worst


def _window(n_fft):
    return R.hann(n_fft).to(torch.float32)


# ---- stft_frames ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nonfinite", [False, True])
@pytest.mark.parametrize("n_fft,hop,B,T", SHAPES)
def test_stft_frames_bit_equal(n_fft, hop, B, T, nonfinite, dev):
    """window[f] * x[...] is exact in float64, so one rounding to fp32 gives the kernel's bits; columns outside the written
    range keep their contents; every entry drawn from a non-finite sample is 0."""
    from multimodal_vqvae_compression_audio_tactile_amd import ops
    g = _gen(1, n_fft, B, T)
    x0, x1 = _randn(g, B, T), _randn(g, B, T)
    bad = torch.zeros(B, T, dtype=torch.bool)
    if nonfinite:
        for i, t in enumerate((0, 1, T - 2, T - 1, T // 2)):
            x0[i % B, t] = NONFINITE[i % 3]; bad[i % B, t] = True
    w = _window(n_fft)
    nfr = R.nframes(T, hop)
    Nh = B * nfr
    sentinel = -2.0 ** 33
    plane = torch.full((n_fft, 2 * Nh + 5), sentinel, dtype=torch.float32, device=dev)
    ops.stft_frames(x0.to(dev), w.to(dev), plane, 0, n_fft, hop)
    want0 = R.stft_frames(x0, w, n_fft, hop).reshape(n_fft, Nh).to(torch.float32)
    got = plane.cpu()
    assert _bits_equal(got[:, :Nh], want0)
    assert bool((got[:, Nh:] == sentinel).all())
    ops.stft_frames(x1.to(dev), w.to(dev), plane, Nh, n_fft, hop)
    got = plane.cpu()
    assert _bits_equal(got[:, :Nh], want0)
    assert _bits_equal(got[:, Nh:2 * Nh], R.stft_frames(x1, w, n_fft, hop).reshape(n_fft, Nh).to(torch.float32))
    assert bool((got[:, 2 * Nh:] == sentinel).all())
    if nonfinite:
        drawn = bad[:, R.frame_index(T, n_fft, hop)].permute(1, 0, 2).reshape(n_fft, Nh)
        assert int(drawn.sum()) > 5 and bool((got[:, :Nh][drawn] == 0).all())


# ---- the DFT GEMM --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncols", [6, 264])
@pytest.mark.parametrize("n_fft", [256, 512, 1024])
def test_dft_gemm(n_fft, ncols, dev):
    from multimodal_vqvae_compression_audio_tactile_amd import losses, ops
    plan = losses._SpecPlan.get(n_fft, dev)
    W, F, Fp = R.padded_basis(n_fft)
    W = W.to(torch.float32).to(F64)                                      # the fp32 basis the plan packed
    assert (F, Fp) == (plan.F, plan.Fp)
    fr = _randn(_gen(2, n_fft, ncols), n_fft, ncols)
    S = ops.conv1d(fr.to(dev).reshape(1, n_fft, ncols), plan.wp, 2 * Fp, 1)[0].cpu()
    want = W @ fr.to(F64)
    scale = W.abs() @ fr.to(F64).abs()
    _ratio(f"dft_gemm[{n_fft},{ncols}]", S, want, U * scale, n_fft)
    assert bool((S[F:Fp] == 0).all()) and bool((S[Fp + F:] == 0).all())


# ---- spec_mag ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncols", [6, 528])
def test_spec_mag(ncols, dev):
    from multimodal_vqvae_compression_audio_tactile_amd import ops
    F, Fp, eps = 129, 160, R.f32(1e-7)
    g = _gen(3, ncols)
    S = _randn(g, 2 * Fp, ncols) * torch.exp(math.log(2e3) * (2 * _rand(g, 1, ncols) - 1))      # column scales 5e-4 .. 2e3
    S[:, 1] = 0.0                                                                                 # a silent column
    S[:, 2] = 1e-7 * (0.2 + 1.6 * _rand(g, 2 * Fp)) / math.sqrt(2.0)                             # |z| straddles eps
    S[5, 3] = 2e3; S[Fp + 5, 3] = -2e3
    mag = ops.spec_mag(S.to(dev).reshape(1, 2 * Fp, ncols), F, Fp, 1e-7).cpu()
    re, im = S[:F], S[Fp:Fp + F]
    raw = (re.to(F64) ** 2 + im.to(F64) ** 2).sqrt()
    want = R.spec_mag(re, im, eps)
    _ratio(f"spec_mag[{ncols}]", mag[:F], want, U * want, 6)
    below = raw < eps * (1 - 6 * U)
    assert int(below[:, 2].sum()) > 10 and int((~below[:, 2]).sum()) > 10 and bool(below[:, 1].all())
    assert bool((mag[:F][below] == eps).all())
    assert bool((mag[F:] == 0).all())


# ---- spec_loss_sums ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,nfr,B", [(129, 3, 1), (257, 6, 3), (513, 94, 2)])
def test_spec_loss_sums(F, nfr, B, dev):
    """(129,3,1): 387 elements, so all but the first two of the 16 partial blocks have none and must contribute 0."""
    from multimodal_vqvae_compression_audio_tactile_amd import ops
    Fp = (F + 31) // 32 * 32
    g = _gen(4, F, nfr, B)
    mag = torch.empty(Fp, 2, B, nfr)
    mag[:, 0] = 0.5 + _rand(g, Fp, B, nfr)                               # prediction half: 0.5 .. 1.5
    mag[:, 1] = 3.0 * _rand(g, Fp, B, nfr) * (1 + torch.arange(B).reshape(1, B, 1))      # target half: wider, per item
    mag[F:] = 1e6                                                        # padded rows are not part of any sum
    got = ops.spec_loss_sums(mag.reshape(Fp, 2 * B * nfr).to(dev), F, B, nfr).cpu()
    want = R.spec_loss_sums(mag[:F, 0], mag[:F, 1])
    k = 3 + -(-F * nfr // 4096) + 8 + 9
    _ratio(f"spec_loss_sums[{F},{nfr},{B}]", got, want, U * want, k)


# ---- spec_grad -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coef_b", [0.0, 3.7e-4])
@pytest.mark.parametrize("with_extra", [False, True])
@pytest.mark.parametrize("with_a", [False, True])
def test_spec_grad(with_a, with_extra, coef_b, dev):
    from multimodal_vqvae_compression_audio_tactile_amd import ops
    F, Fp, B, nfr, eps = 257, 288, 3, 94, 2.0 ** -23
    half = B * nfr
    g = _gen(5, int(with_a), int(with_extra))
    S = _randn(g, 2 * Fp, 2, B, nfr)
    mag = torch.empty(Fp, 2, B, nfr)
    mag[:, 0] = 0.5 + _rand(g, Fp, B, nfr); mag[:, 1] = 2.0 * _rand(g, Fp, B, nfr)
    mag[7, 1, 1, 3] = mag[7, 0, 1, 3]; mag[F - 1, 1, 2, nfr - 1] = mag[F - 1, 0, 2, nfr - 1]     # X == Y: sign 0
    planted = {"below": (9, 0, 2), "at": (11, 2, 90), "zero": (F - 1, 1, 0), "at_last": (0, B - 1, nfr - 1)}
    k_, b_, n_ = planted["below"]; S[k_, 0, b_, n_] = 2.0 ** -25; S[Fp + k_, 0, b_, n_] = 2.0 ** -25      # |z| = 2^-24.5 < eps
    for key in ("at", "at_last"):
        k_, b_, n_ = planted[key]; S[k_, 0, b_, n_] = 2.0 ** -23; S[Fp + k_, 0, b_, n_] = 0.0           # |z| == eps, no rounding
    k_, b_, n_ = planted["zero"]; S[k_, 0, b_, n_] = 0.0; S[Fp + k_, 0, b_, n_] = 0.0
    coef_a = (0.01 + _rand(g, B)) if with_a else None
    extra = _randn(g, Fp, B, nfr) * 1e-3 if with_extra else None
    G = ops.spec_grad(S.reshape(1, 2 * Fp, 2 * half).to(dev), mag.reshape(Fp, 2 * half).to(dev),
                      None if coef_a is None else coef_a.to(dev), coef_b,
                      None if extra is None else extra.reshape(Fp, half).to(dev), F, Fp, B, nfr, eps).cpu()
    G = G.reshape(2 * Fp, B, nfr)
    re, im = S[:F, 0], S[Fp:Fp + F, 0]
    X, Y = mag[:F, 0], mag[:F, 1]
    gre, gim, _ = R.spec_grad(re, im, X, Y, coef_a, R.f32(coef_b), None if extra is None else extra[:F], eps)
    d = X.to(F64) - Y.to(F64)
    sg = R.f32(coef_b) * torch.sign(d).abs()
    if coef_a is not None:
        sg = sg + (coef_a.to(F64).reshape(1, B, 1) * d).abs()
    if extra is not None:
        sg = sg + extra[:F].to(F64).abs()
    a = (re.to(F64) ** 2 + im.to(F64) ** 2).sqrt()
    live = (a >= eps) & (a > 0)
    a1 = torch.where(a > 0, a, torch.ones_like(a))
    excused = ((a - eps).abs() <= 6 * U * a) & (a != eps)                # no such element is planted or expected
    for name, got, want, z in (("re", G[:F], gre, re), ("im", G[Fp:Fp + F], gim, im)):
        scale = torch.where(live, sg * z.to(F64).abs() / a1, torch.zeros_like(a))
        _ratio(f"spec_grad.{name}[a={with_a},extra={with_extra},b={coef_b}]", got, want, U * scale, 12, excused)
    assert not bool(excused.any())
    for key in ("below", "zero"):
        k_, b_, n_ = planted[key]
        assert float(G[k_, b_, n_]) == 0.0 and float(G[Fp + k_, b_, n_]) == 0.0
    if with_a or with_extra or coef_b:
        for key in ("at", "at_last"):                                    # |z| == eps: the gradient passes
            k_, b_, n_ = planted[key]
            assert float(gre[k_, b_, n_]) != 0.0 and float(G[k_, b_, n_]) != 0.0 and float(G[Fp + k_, b_, n_]) == 0.0
    if coef_b and not with_a and not with_extra:
        assert float(G[7, 1, 3]) == 0.0 and float(G[Fp + 7, 1, 3]) == 0.0                        # sign(0) = 0
    assert bool((G[F:Fp] == 0).all()) and bool((G[Fp + F:] == 0).all())


# ---- overlap_add ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("corners_only", [False, True])
@pytest.mark.parametrize("n_fft,hop,B,T", SHAPES)
def test_overlap_add(n_fft, hop, B, T, corners_only, dev):
    """The kernel accumulates into dy, so dy starts random.  corners_only: dF is non-zero in the first and last window taps
    of the first and last frames only -- the contributions an off-by-one in the tap or frame range loses."""
    from multimodal_vqvae_compression_audio_tactile_amd import ops
    g = _gen(6, n_fft, B, T)
    nfr = R.nframes(T, hop)
    dF = _randn(g, n_fft, B, nfr)
    if corners_only:
        keep = torch.zeros(n_fft, 1, nfr)
        for f in (0, n_fft - 1):
            for n in (0, nfr - 1):
                keep[f, 0, n] = 1.0
        dF = dF * keep
    dy0 = _randn(g, B, T)
    # the periodic hann window is 0 at tap 0: a window that is not, so that tap 0 is seen (the kernel takes any window)
    w = (_window(n_fft) + 0.25).contiguous()
    dy = ops.overlap_add_(dy0.clone().to(dev), dF.reshape(n_fft, B * nfr).to(dev), w.to(dev), n_fft, hop).cpu()
    want = R.overlap_add(dF, w, T, hop, dy0)
    scale = R.overlap_add(dF.abs(), w, T, hop, dy0.abs())
    _ratio(f"overlap_add[{n_fft},{hop},{B},{T},corners={corners_only}]", dy, want, U * scale, 3 * n_fft // hop + 2)
    if corners_only:
        untouched = R.overlap_add((dF != 0).to(F64), torch.ones(n_fft), T, hop) == 0
        assert int(untouched.sum()) > 0 and _bits_equal(dy[untouched], dy0[untouched])


# ---- l1_loss_sum ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_dy", [True, False])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1024 * 256 + 3])
def test_l1_loss_sum(n, with_dy, dev):
    """n = 1024*256 + 3: the block count is capped at 1024, so the grid-stride loop takes a second pass.  The gradient is
    dy + coef*sign(d): exact in float64, one rounding, so it is compared bit for bit."""
    from multimodal_vqvae_compression_audio_tactile_amd import ops
    g = _gen(7, n)
    y, tgt = _randn(g, n), _randn(g, n)
    if n >= 255:
        y[0] = tgt[0]; y[200] = tgt[200]
        y[3] = NONFINITE[0]; tgt[5] = NONFINITE[1]; y[7] = NONFINITE[2]; tgt[7] = NONFINITE[0]
        tgt[9] = NONFINITE[2]; y[n - 1] = NONFINITE[1]
    dy0 = _randn(g, n)
    coef = 0.55 / n
    dyd = dy0.clone().to(dev) if with_dy else None
    got = ops.l1_loss_sum(y.to(dev), tgt.to(dev), dyd, coef if with_dy else 0.0).cpu()
    want, sign = R.l1_loss(y, tgt)
    P = max(1, min(1024, (n + 255) // 256))
    k = 1 + -(-n // (256 * P)) + 8 + -(-P // 256) + 8
    _ratio(f"l1_loss_sum[{n},dy={with_dy}]", got, want, U * want, k)
    if with_dy:
        want_dy = (dy0.to(F64) + R.f32(coef) * sign).to(torch.float32)
        assert _bits_equal(dyd, want_dy)
        if n >= 255:
            assert _bits_equal(dyd[[0, 200, 7]], dy0[[0, 200, 7]])       # y == tgt (after sanitising): untouched


# ---- mel_max -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("B,nfr", [(1, 3), (3, 6), (3, 94)])
def test_mel_max_first_of_ties(B, nfr, variant, dev):
    """Exact maximum and the row-major-first argmax.  Ties are planted per (half, item): within one mel row; the last frame
    of row 3 against the first frame of row 4; elements 7 and 135, whose threads meet only in the last tree level; and a
    pair whose first element sits in the higher thread (or, with too few elements for that, the first and the last).  (1,3) has 192 elements: fewer than the block has threads."""
    from multimodal_vqvae_compression_audio_tactile_amd import ops
    n_mels = 64
    g = _gen(8, B, nfr, variant)
    M = _rand(g, n_mels, 2, B, nfr)
    total = n_mels * nfr
    ties = [(5 * nfr, 5 * nfr + nfr - 1), (3 * nfr + nfr - 1, 4 * nfr), (7, 135), (200, 266) if total > 266 else (0, total - 1)]
    for slot in range(2 * B):
        e0, e1 = ties[(slot + variant * 2) % 4]
        h, b = divmod(slot, B)
        for e in (e0, e1):
            M[e // nfr, h, b, e % nfr] = 2.0 + slot
    maxv, argm = ops.mel_max(M.reshape(1, n_mels, 2 * B * nfr).to(dev), n_mels, B, nfr)
    wv = torch.cat([R.mel_max(M[:, 0])[0], R.mel_max(M[:, 1])[0]])
    wa = torch.cat([R.mel_max(M[:, 0])[1], R.mel_max(M[:, 1])[1]])
    assert [int(a) for a in wa] == [ties[(s + variant * 2) % 4][0] for s in range(2 * B)]
    assert len(set(int(a) for a in wa)) > 1                              # the two halves peak at different places
    assert _bits_equal(maxv, wv)
    assert [int(a) for a in argm.cpu()] == [int(a) for a in wa]


# ---- mel_cos -------------------------------------------------------------------------------------------------------------
def _mel_cos_bounds(Mx, My, maxx, maxy, eps, use_log, coef):
    """First-order propagation of the fp32 roundings of mel_cos_kernel, operation by operation, in units of u: each
    returned bound is u * sum over the operations of (roundings of the operation) * |its contribution to the result|."""
    Mx, My = Mx.to(F64), My.to(F64)
    n_mels, B, nfr = Mx.shape
    denx = maxx.to(F64).clamp_min(eps).reshape(1, B, 1); deny = maxy.to(F64).clamp_min(eps).reshape(1, B, 1)
    if use_log:
        ux, uy = Mx / denx + eps, My / deny + eps
        X, Y = ux.log(), uy.log()
        eX, eY = U * (2 + 4 * X.abs()), U * (2 + 4 * Y.abs())           # division, add: 2u relative on the argument; logf 2 ulp
    else:
        ux = uy = None
        X, Y = Mx / denx, My / deny
        eX, eY = U * X.abs(), U * Y.abs()
    nd = n_mels + 1                                                      # a product and n_mels serial adds
    num = (X * Y).sum(0)
    e_num = (eX * Y.abs() + eY * X.abs()).sum(0) + nd * U * (X * Y).abs().sum(0)
    nx2, ny2 = (X * X).sum(0), (Y * Y).sum(0)
    nx, ny = nx2.sqrt(), ny2.sqrt()
    tiny = 1e-300
    e_nx = ((2 * X.abs() * eX).sum(0) + nd * U * nx2) / (2 * nx).clamp_min(tiny) + 4 * U * nx
    e_ny = ((2 * Y.abs() * eY).sum(0) + nd * U * ny2) / (2 * ny).clamp_min(tiny) + 4 * U * ny
    prod = nx * ny
    e_prod = e_nx * ny + e_ny * nx + U * prod
    den2 = prod.clamp_min(eps)
    e_den = torch.where(prod >= eps, e_prod, torch.zeros_like(prod))
    v = num / den2
    e_v = e_num / den2 + num.abs() * e_den / den2 ** 2 + U * v.abs()
    if coef is None or not use_log:
        return v, e_v, None, None
    gnum = coef / den2
    e_gnum = gnum.abs() * (e_den / den2 + U)
    gprod = torch.where(prod >= eps, -coef * num / den2 ** 2, torch.zeros_like(prod))
    e_gprod = torch.where(prod >= eps, abs(coef) * (e_num / den2 ** 2 + 2 * num.abs() * e_den / den2 ** 3) + 3 * U * gprod.abs(),
                          torch.zeros_like(prod))
    nx_ = nx.clamp_min(tiny)
    t1, t2 = gnum * Y, gprod * ny * X / nx_
    e_t2 = (e_gprod * ny * X.abs() / nx_ + gprod.abs() * (e_ny * X.abs() / nx_ + ny * eX / nx_ + ny * X.abs() * e_nx / nx_ ** 2)
            + 3 * U * t2.abs())
    gX = t1 + t2
    e_gX = e_gnum * Y.abs() + gnum.abs() * eY + U * t1.abs() + e_t2 + U * (t1.abs() + t2.abs())
    gu = gX / ux
    e_gu = e_gX / ux + gX.abs() * (2 * U * ux) / ux ** 2 + U * gu.abs()
    dM = gu / denx
    e_dM = e_gu / denx + U * dM.abs()
    term = gu * Mx / denx ** 2
    e_dden = (e_gu * Mx / denx ** 2 + 3 * U * term.abs()).sum(0) + n_mels * U * term.abs().sum(0)
    return v, e_v, e_dM, e_dden


@pytest.mark.parametrize("eps", [1e-7, 1e-8])
@pytest.mark.parametrize("use_log", [True, False])
def test_mel_cos(use_log, eps, dev):
    """M spans 1e-9 .. 1; item 1 lies entirely below eps (the clamp on the maximum applies); in item 0 one frame's prediction
    column equals its target column and holds both maxima, so cos = 1 at the clamp(-1, 1) gate; with use_log off one
    column is silent (|X||Y| < eps).  Without coef neither gradient buffer is written; with it (use_log only) dM and dden
    match float64 autograd of the forward formula."""
    from multimodal_vqvae_compression_audio_tactile_amd import ops
    n_mels, B, nfr = 64, 3, 94
    half = B * nfr
    e32 = R.f32(eps)
    g = _gen(9, int(use_log), int(eps * 1e9))
    M = torch.exp(math.log(1e-9) * _rand(g, n_mels, 2, B, nfr))          # log-uniform on 1e-9 .. 1
    M[:, :, 1] = e32 * (0.01 + 0.89 * _rand(g, n_mels, 2, nfr))          # an item below eps in both halves
    M[:, 1, 0, 40] = M[:, 0, 0, 40]
    M[20, :, 0, 40] = 1.5                                                # ... which holds the maximum of both halves
    if not use_log:
        M[:, 0, 2, 5] = 0.0
    maxx, maxy = R.mel_max(M[:, 0])[0], R.mel_max(M[:, 1])[0]
    assert float(maxx[1]) < e32 and float(maxx[0]) == 1.5 == float(maxy[0])
    maxv = torch.cat([maxx, maxy]).to(dev)
    Md = M.reshape(1, n_mels, 2 * half).to(dev)
    coef = -0.2 / half
    cos0, dM0, dden0 = ops.mel_cos(Md, maxv, n_mels, B, nfr, eps, coef=None, use_log=use_log)
    assert dM0 is None and dden0 is None
    v, e_v, e_dM, e_dden = _mel_cos_bounds(M[:, 0], M[:, 1], maxx, maxy, e32, use_log, R.f32(coef) if use_log else None)
    want_cos, want_dM, want_dden = R.mel_cos(M[:, 0], M[:, 1], maxx, maxy, e32, use_log, R.f32(coef) if use_log else None)
    name = f"mel_cos[log={use_log},eps={eps}]"
    _ratio(name + ".cos", cos0.reshape(B, nfr), want_cos, e_v, 1)
    assert abs(float(want_cos[0, 40]) - 1.0) < 1e-12
    if not use_log:
        assert float(cos0.reshape(B, nfr)[2, 5]) == 0.0
        return
    cos1, dM, dden = ops.mel_cos(Md, maxv, n_mels, B, nfr, eps, coef=coef, use_log=True)
    assert _bits_equal(cos1, cos0.cpu())
    # a column whose float64 v is within its bound of +-1 may be cut by the clamp or not: the other branch is accepted there
    gate = (v.abs() - 1.0).abs() <= e_v
    assert bool(gate[0, 40]) and int(gate.sum()) <= 0.01 * gate.numel()
    _, in_dM, in_dden = R.mel_cos(M[:, 0], M[:, 1], maxx, maxy, e32, True, R.f32(coef), clamp_grad=False)
    dM, dden = dM.cpu().reshape(n_mels, B, nfr).to(F64), dden.cpu().reshape(B, nfr).to(F64)
    for nm, got, want, inside, bound in (("dM", dM, want_dM, in_dM, e_dM), ("dden", dden, want_dden, in_dden, e_dden)):
        gt = gate.expand_as(got)
        err = (got - want).abs()
        err = torch.where(gt, torch.minimum(err, torch.minimum((got - inside).abs(), got.abs())), err)
        _ratio(f"{name}.{nm}", got, want, bound, 1, err=err)


# ---- mel_max_grad_ -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nfr", [3, 300])
def test_mel_max_grad(nfr, dev):
    """Item 0: max well above eps; item 1: max below eps, nothing moves; item 2: max == eps exactly, updated.  Only the
    argmax element of an updated item changes, by the sum of its item's dden."""
    from multimodal_vqvae_compression_audio_tactile_amd import ops
    n_mels, B, eps = 64, 3, 1e-7
    e32 = np.float32(eps)
    g = _gen(10, nfr)
    dM0 = _randn(g, n_mels, B, nfr)
    dden = _randn(g, B, nfr)
    maxv = torch.tensor([0.7, float(e32) * 0.999, float(e32), 9.0, 9.0, 9.0], dtype=torch.float32)
    argm = torch.tensor([n_mels * nfr - 1, 5, 17 * nfr + nfr // 2, 0, 0, 0], dtype=torch.int32)
    got = ops.mel_max_grad_(dM0.clone().reshape(n_mels, B * nfr).to(dev), dden.reshape(B * nfr).to(dev), maxv.to(dev),
                            argm.to(dev), B, nfr, eps).cpu().reshape(n_mels, B, nfr)
    want = R.mel_max_grad(dM0, dden, maxv, argm, float(e32))
    touched = torch.zeros(n_mels, B, nfr, dtype=torch.bool)
    scale = torch.zeros(n_mels, B, nfr, dtype=F64)
    for b in (0, 2):
        e = int(argm[b])
        touched[e // nfr, b, e % nfr] = True
        scale[e // nfr, b, e % nfr] = dden[b].to(F64).abs().sum() + abs(float(dM0[e // nfr, b, e % nfr]))
    assert _bits_equal(got[~touched], dM0[~touched])
    assert bool((got[touched] != dM0[touched]).all())
    _ratio(f"mel_max_grad[{nfr}]", got[touched], want[touched], U * scale[touched], -(-nfr // 256) + 8 + 1)


# ---- what the C entry points refuse before any launch ----------------------------------------------------------------------
@pytest.mark.parametrize("which,T", [("stft", 128), ("mel", 256), ("mel", 100)])
def test_too_short_clips_are_refused(which, T, dev):
    """Reflect padding needs T > n_fft/2; the reference raises at these lengths too."""
    from multimodal_vqvae_compression_audio_tactile_amd import losses
    from multimodal_vqvae_compression_audio_tactile_amd.ops import MvqError
    y = _randn(_gen(11, T), 2, 1, T).to(dev)
    crit = losses.MultiResSTFTLoss() if which == "stft" else losses.MelCosineLoss()
    with pytest.raises(MvqError):
        crit(y, y.clone())


# ---- zero gradient at non-finite prediction samples ------------------------------------------------------------------------
def _rel(got, want):
    got = got.detach().double().cpu().reshape(-1); want = want.detach().double().cpu().reshape(-1)
    return float((got - want).norm() / want.norm().clamp_min(1e-30))


@pytest.fixture(scope="module")
def masked_signals():
    from multimodal_vqvae_compression_audio_tactile_amd import synth
    B, T = 2, 4000
    g = torch.Generator().manual_seed(5)
    tgt = synth.tactile_segments(B, seed=5, T=T) + 1e-3 * torch.randn(B, 1, T, generator=g)       # as test_gpu_losses._signals
    y = tgt + 0.05 * torch.randn(B, 1, T, generator=g)
    for i, (b, t) in enumerate(((0, 0), (0, 17), (1, T - 1), (1, 17), (1, 0), (0, T - 1))):
        y[b, 0, t] = NONFINITE[i % 3]
    return y, tgt


@torch.enable_grad()
@pytest.mark.parametrize("name", ["safe_l1", "mrstft", "total"])
def test_zero_gradient_at_non_finite_samples(name, masked_signals, dev):
    """nan_to_num's autograd gives a non-finite prediction sample gradient 0; so does every loss here, exactly.  Elsewhere
    value and gradient agree with the oracle at the suite's bars (1e-4, 1e-3 relative L2).  The reference's MelCosineLoss
    returns NaN on such input; here the mel term sanitises, so the total is compared on nan_to_num(y)."""
    from oracle import losses_torch as LT
    from multimodal_vqvae_compression_audio_tactile_amd import losses
    y, tgt = masked_signals
    bad = ~torch.isfinite(y)
    assert int(bad.sum()) == 6
    if name == "total":
        yr = LT.finite_or_zero(y).requires_grad_(True)
        want = LT.total_loss(yr, tgt)[0]
        mine = losses.TrainingLoss().to(dev)
    else:
        yr = y.clone().requires_grad_(True)
        want = (LT.safe_l1 if name == "safe_l1" else LT.mrstft)(yr, tgt)
        mine = losses.safe_l1 if name == "safe_l1" else losses.MultiResSTFTLoss().to(dev)
    want.backward()
    yd = y.to(dev).requires_grad_(True)
    got = mine(yd, tgt.to(dev)); got.backward()
    grad = yd.grad.cpu()
    assert bool((grad[bad] == 0).all()), grad[bad]
    assert bool(torch.isfinite(grad).all())
    ref = torch.where(bad, torch.zeros_like(yr.grad), yr.grad)
    err = _rel(grad, ref)
    print(f"{name}: value {float(got.detach()):.7g} vs {float(want.detach()):.7g}, dL/dy relative L2 {err:.2e}")
    assert abs(float(got) - float(want)) <= 1e-4 * abs(float(want)) + 1e-7
    assert err < 1e-3
