"""-m gpu: backward kernels of the trainable head (kernels_bwd.hip, ops.linear_wgrad) at the shapes the training step runs --
C = 1024 LayerNorms over one AR chunk of 6 or 256 segments (the <4, 64> and <16, 64> register forms), 8-head attention with
dh = 128, weight gradients with K = 66 ... 4 096 tokens -- against float64 torch autograd.

These rows are tolerance-checked by design (kernels_bwd.hip header).  Each tensor keeps the suite's bar, relative L2 error
<= TOL = 2e-4, and in addition the WORST token (column) of an activation gradient, the worst row / column of a weight gradient and
the worst element of a per-channel gradient (relative to the tensor's RMS) must stay <= WORST = 2e-5.  The whole-tensor norm alone
is blind to a local error: at 4 096 tokens one token off by 1 % moves it by ~1.6e-4.  Largest values measured on the MI355X over
every shape below: LayerNorm gx per token 1.9e-7, dgamma / dbeta per element 5.3e-7, attention per token 8.1e-7, weight gradient
per row 2.2e-6 (fp32 chains over up to 4 129 tokens).  2e-5 is ~10x the largest of them and still flags one token, row or
channel that is off by 0.01 %."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
TOL = 2e-4
WORST = 2e-5


def rel(got, want):
    got = got.detach().double().cpu().reshape(-1); want = want.detach().double().cpu().reshape(-1)
    return float((got - want).norm() / want.norm().clamp_min(1e-30))


def worst_slice(got, want, dim):
    """Largest relative L2 error over the slices got.select(dim, i) (one token, one row, ...)."""
    d = (got.detach().double().cpu() - want.detach().double().cpu()).movedim(dim, 0).reshape(got.shape[dim], -1)
    w = want.detach().double().cpu().movedim(dim, 0).reshape(got.shape[dim], -1)
    return float((d.norm(dim=1) / w.norm(dim=1).clamp_min(1e-30)).max())


def worst_elem(got, want):
    """Largest element error relative to the tensor's RMS (per-channel gradients: a sum over tokens can be near zero)."""
    got = got.detach().double().cpu(); want = want.detach().double().cpu()
    return float((got - want).abs().max() / want.pow(2).mean().sqrt().clamp_min(1e-30))


def tokens(x, B):
    """[B, C, T] or the folded [1, C, B*T] -> [C, B*T]: one column per token."""
    if x.shape[0] == 1:
        return x[0]
    return x.permute(1, 0, 2).reshape(x.shape[1], -1)


def fold(x):
    B, C, T = x.shape
    return x.permute(1, 0, 2).reshape(1, C, B * T).contiguous()


def check(name, got, want, per_token_dim=None, per_elem=False):
    assert torch.isfinite(got).all(), name
    r = rel(got, want)
    assert r <= TOL, f"{name}: relative L2 error {r:.3g} > {TOL}"
    if per_token_dim is not None:
        w = worst_slice(got, want, per_token_dim)
        assert w <= WORST, f"{name}: worst slice relative error {w:.3g} > {WORST}"
    if per_elem:
        w = worst_elem(got, want)
        assert w <= WORST, f"{name}: worst element error / RMS {w:.3g} > {WORST}"


# ----------------------------------------------------------------------------------------------------------------- LayerNorm
# (B, T) with n = B * T tokens: 1, 3, the AR chunks at B = 6 (66, 96), both sides of the <4, 64> / <16, 64> switch at 1 024, the
# AR chunks at B = 256 (2 816 = 256 x 11, 4 101 = 4 096 + 5: a partial last block of 16 tokens)
LN_SHAPES = [(1, 1), (3, 1), (6, 11), (6, 16), (3, 341), (64, 16), (5, 205), (256, 11), (3, 1367)]


def _ln_case(B, T, C, use_pe, folded, seed, dev):
    from multimodal_vqvae_compression_audio_tactile_amd import ops, synth
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, T, generator=g, dtype=torch.float64) * 1.5 + 0.3
    gam = 1 + 0.2 * torch.randn(C, generator=g, dtype=torch.float64)
    bet = 0.1 * torch.randn(C, generator=g, dtype=torch.float64)
    go = torch.randn(B, C, T, generator=g, dtype=torch.float64)
    pe = synth.pos_table(C, max(T, 16)) if use_pe else None
    xr, gr, br = (t.clone().requires_grad_(True) for t in (x, gam, bet))
    xin = xr + pe[:T].T.double().unsqueeze(0) if use_pe else xr
    u = F.layer_norm(xin.permute(0, 2, 1), (C,), gr, br, 1e-5).permute(0, 2, 1)
    (u * go).sum().backward()
    xd = (fold(x) if folded else x).float().to(dev)
    gd = (fold(go) if folded else go).float().to(dev)
    ped = pe[:T].contiguous().to(dev) if use_pe else None
    gamd = gam.float().to(dev)
    kw = dict(pe=ped, eps=1e-5, folded_batch=B if folded else None)
    gx, dgam, dbet = ops.layernorm_c_bwd(xd, gamd, gd, **kw)
    _, dgam2, dbet2 = ops.layernorm_c_bwd(xd, gamd, gd, need_gx=False, **kw)
    torch.cuda.synchronize()
    return (tokens(gx.cpu(), B), tokens(xr.grad, B)), (dgam.cpu(), gr.grad), (dbet.cpu(), br.grad), (dgam2.cpu(), dbet2.cpu())


@pytest.mark.parametrize("B,T", LN_SHAPES, ids=[f"n{B * T}" for B, T in LN_SHAPES])
def test_layernorm_backward_at_c1024(B, T, dev):
    """ops.layernorm_c_bwd at the predictor width: folded (as train.LayerNormC calls it) and unfolded, with and without the
    positional table; need_gx=False gives the same parameter gradients bit for bit."""
    for folded in (True, False):
        for use_pe in (True, False):
            tag = f"n={B * T} folded={folded} pe={use_pe}"
            gx, dgam, dbet, (dgam2, dbet2) = _ln_case(B, T, 1024, use_pe, folded, seed=B * 1000 + T + 2 * folded + use_pe, dev=dev)
            check(f"gx {tag}", *gx, per_token_dim=1)
            check(f"dgamma {tag}", *dgam, per_elem=True)
            check(f"dbeta {tag}", *dbet, per_elem=True)
            assert torch.equal(dgam2, dgam[0]) and torch.equal(dbet2, dbet[0]), tag


def test_layernorm_backward_generic_width_many_tokens(dev):
    """C = 96 (the generic kernel, 16 tokens per block) at an AR chunk of 256 segments plus a partial last block."""
    for folded in (True, False):
        gx, dgam, dbet, _ = _ln_case(3, 1367, 96, True, folded, seed=96 + folded, dev=dev)
        check(f"gx folded={folded}", *gx, per_token_dim=1)
        check(f"dgamma folded={folded}", *dgam, per_elem=True)
        check(f"dbeta folded={folded}", *dbet, per_elem=True)


# ----------------------------------------------------------------------------------------------------------------- attention
def _attention_case(B, T, dev, H=8, dh=128, seed=0):
    from multimodal_vqvae_compression_audio_tactile_amd import ops
    g = torch.Generator().manual_seed(seed)
    C = H * dh
    q, k, v = (torch.randn(B, C, T, generator=g, dtype=torch.float64) for _ in range(3))
    go = torch.randn(B, C, T, generator=g, dtype=torch.float64)
    qr, kr, vr = (t.clone().requires_grad_(True) for t in (q, k, v))
    sp = lambda x: x.permute(0, 2, 1).reshape(B, -1, H, dh).permute(0, 2, 1, 3)
    att = (sp(qr) @ sp(kr).transpose(-2, -1)) / math.sqrt(dh)
    ctx = (att.softmax(-1) @ sp(vr)).permute(0, 2, 1, 3).reshape(B, T, C).permute(0, 2, 1)
    (ctx * go).sum().backward()
    gq, gk, gv = ops.attention_bwd(*(fold(t).float().to(dev) for t in (q, k, v, go)), H, folded_batch=B)
    torch.cuda.synchronize()
    return [(tokens(got.cpu(), B), tokens(want, B)) for got, want in ((gq, qr.grad), (gk, kr.grad), (gv, vr.grad))]


@pytest.mark.parametrize("B,T", [(6, 16), (6, 11), (256, 16), (256, 11), (6, 28)])
def test_attention_backward_at_the_predictor_width(B, T, dev):
    """ops.attention_bwd with 8 heads of dh = 128 (c = 1024) over the AR chunks (16 / 11 tokens) at B = 6 and 256, folded layout,
    and at Tq = Tk = 28, the longest window whose operands fit the launcher's 64 KB of LDS at dh = 128."""
    for name, (got, want) in zip(("gq", "gk", "gv"), _attention_case(B, T, dev, seed=B * 100 + T)):
        check(f"{name} B={B} T={T}", got, want, per_token_dim=1)


def test_attention_backward_refuses_what_does_not_fit(dev):
    """Tq = Tk = 32 at dh = 128 needs 72 KB of LDS: refused with MvqError before any launch (the stream stays clean)."""
    from multimodal_vqvae_compression_audio_tactile_amd import ops
    from multimodal_vqvae_compression_audio_tactile_amd._lib import MvqError
    B, T, C = 2, 32, 1024
    q = torch.randn(1, C, B * T, device=dev)
    with pytest.raises(MvqError):
        ops.attention_bwd(q, q, q, q, 8, folded_batch=B)
    torch.cuda.synchronize()
    with pytest.raises(MvqError):
        ops.attention_bwd(q[..., :33].contiguous(), q[..., :33].contiguous(), q[..., :33].contiguous(), q[..., :33].contiguous(), 8)
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------------------- weight gradient
WGRAD_PAIRS = [(1024, 1024), (2048, 1024), (1024, 2048), (96, 1024), (1024, 96)]
WGRAD_N = [66, 96, 2816, 4096, 4129]          # B x 11 / B x 16 tokens at B = 6 and 256; 4 129 = 129 x 32 + 1


@pytest.mark.parametrize("O,I", WGRAD_PAIRS, ids=[f"{o}x{i}" for o, i in WGRAD_PAIRS])
def test_linear_wgrad_at_training_token_counts(O, I, dev):
    """dW = g x^T over N tokens (the conv MFMA kernel with K = tokens; N % 32 != 0 takes the zero-padded path) against a float64
    product, for the predictor's (O, I) pairs."""
    from multimodal_vqvae_compression_audio_tactile_amd import ops
    for N in WGRAD_N:
        gen = torch.Generator().manual_seed(O * 7 + I + N)
        g = torch.randn(O, N, generator=gen)
        x = torch.randn(I, N, generator=gen)
        got = ops.linear_wgrad(g.to(dev), x.to(dev))
        want = (g.double().to(dev) @ x.double().to(dev).T).cpu()
        assert got.shape == (O, I)
        check(f"dW {O}x{I} N={N}", got.cpu(), want, per_token_dim=0)
        check(f"dW^T {O}x{I} N={N}", got.cpu(), want, per_token_dim=1)
