"""-m gpu: training under the lossy link -- the masked attention backward kernels (chunk and sequence form), the device loss
draw, and the whole AllPredAR / AllPredPLC training step on what the receiver reconstructs under loss on both streams.

Kernel contract (include/mvq.h): under a key mask gq is, bit for bit, the existing unmasked backward on the item's K / V compacted
to its present keys, gk / gv at a present column are that launch's values at the column's slot, and gk / gv at an absent column
are +0.  Gradients of the whole step are compared with torch autograd on the restatement (tests/link_train_oracle.py) at the
suite's bar, relative L2 <= 2e-4 per tensor."""
import math

import numpy as np
import pytest
import torch

import link_train_oracle as lt
from multimodal_vqvae_compression_audio_tactile_amd import packets

pytestmark = pytest.mark.gpu
TOL = 2e-4
f32 = np.float32
EINVAL = -1
O = lt.O
_CACHE = {}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _t(dev, *xs):
    return [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in xs]


def rel(got, want):
    got = got.detach().double().cpu().reshape(-1); want = want.detach().double().cpu().reshape(-1)
    return float((got - want).norm() / want.norm().clamp_min(1e-30))


def fold(x):
    B, C, T = x.shape
    return x.permute(1, 0, 2).reshape(1, C, B * T).contiguous()


def unfold(x, B):
    _, C, N = x.shape
    return x.reshape(C, B, N // B).permute(1, 0, 2)


def _masks(B, Tk, seed):
    """The six masks, uint8 [B, Tk]; present keys carry different nonzero values (any nonzero byte is "present")."""
    r = np.random.default_rng(seed)
    m = {"all": np.full((B, Tk), 1, np.uint8), "none": np.zeros((B, Tk), np.uint8)}
    m["first"] = np.zeros((B, Tk), np.uint8); m["first"][:, 0] = 32
    m["last"] = np.zeros((B, Tk), np.uint8); m["last"][:, Tk - 1] = 255
    m["alternating"] = np.tile((np.arange(Tk) % 2 == 0).astype(np.uint8) * 9, (B, 1))
    per = (r.uniform(size=(B, Tk)) < 0.5).astype(np.uint8) * r.integers(1, 256, size=(B, Tk)).astype(np.uint8)
    per[0, 0], per[1 % B, 0] = 0, (1 if B > 1 else 0)                    # rows differ: a wrong m_stride_b shows
    if B > 2:
        per[2] = 0                                                       # one item without a key among items with some
    m["per_item"] = per
    return m


def _seq_masks(B, Tk, seed):
    m = _masks(B, Tk, seed)
    if Tk > 128:                                                         # keys 64..127 entirely, and a partial first tile
        r = np.random.default_rng(seed)
        t = np.ones((B, Tk), np.uint8)
        t[:, 64:128] = 0
        t[:, :64] = r.uniform(size=(B, 64)) < 0.5
        t[:, 40] = 1
        m["tiles"] = t
        o = np.zeros((B, Tk), np.uint8)                                   # only the short last tile has keys
        o[:, 128:] = 1
        m["tail_tile"] = o
    return m


def _qkvg(B, C, Tq, Tk, seed, dev):
    r = np.random.default_rng(seed)
    return _t(dev, *(r.standard_normal((B, C, n)).astype(f32) for n in (Tq, Tk, Tk, Tq)))


def _compacted_bwd(bwd, q, k, v, g, mask, heads):
    """The existing unmasked backward per item on index_select-compacted K / V; gk / gv scattered back, +0 elsewhere.  An item
    without a key: gq = +0 (its ctx does not depend on q)."""
    gq, gk, gv = torch.zeros_like(q), torch.zeros_like(k), torch.zeros_like(v)
    for b in range(q.shape[0]):
        J = torch.nonzero(mask[b] != 0).reshape(-1)
        if J.numel() == 0:
            continue
        a, kk, vv = bwd(q[b:b + 1].contiguous(), k[b:b + 1].index_select(2, J).contiguous(), v[b:b + 1].index_select(2, J).contiguous(),
                        g[b:b + 1].contiguous(), heads)
        gq[b] = a[0]
        gk[b].index_copy_(1, J, kk[0])
        gv[b].index_copy_(1, J, vv[0])
    return gq, gk, gv


def _nan_outputs(lib_call, q, k, v):
    """Run a raw C entry point on outputs pre-filled with NaN -> (rc, gq, gk, gv)."""
    outs = [torch.full_like(x, float("nan")) for x in (q, k, v)]
    return (lib_call(*outs), *outs)


def _chunk_raw(q, k, v, md, g, H, ms=None):
    from multimodal_vqvae_compression_audio_tactile_amd import _lib
    B, C, Tq = q.shape
    Tk = k.shape[2]
    call = lambda gq, gk, gv: _lib.lib().mvq_attention_masked_bwd_f32(
        q.data_ptr(), k.data_ptr(), v.data_ptr(), None if md is None else md.data_ptr(), g.data_ptr(), gq.data_ptr(), gk.data_ptr(),
        gv.data_ptr(), B, H, C // H, Tq, Tk, 0, 0, 0, 0, Tk if ms is None else ms, _stream())
    return _nan_outputs(call, q, k, v)


def _seq_raw(q, k, v, md, g, H, shape=None):
    from multimodal_vqvae_compression_audio_tactile_amd import _lib
    B, C, Tq = q.shape
    Tk = k.shape[2]
    dims = shape or (B, H, C // H, Tq, Tk)
    scratch = torch.empty(max(2 * B * H * Tq * Tk, 4), device=q.device)
    call = lambda gq, gk, gv: _lib.lib().mvq_attention_seq_masked_bwd_f32(
        q.data_ptr(), k.data_ptr(), v.data_ptr(), None if md is None else md.data_ptr(), g.data_ptr(), gq.data_ptr(), gk.data_ptr(),
        gv.data_ptr(), scratch.data_ptr(), *dims, 0, 0, 0, 0, Tk, _stream())
    return _nan_outputs(call, q, k, v)


def _check_against_compacted(got, want, md, k, name):
    for x, w, what in zip(got, want, ("gq", "gk", "gv")):
        assert torch.equal(x, w), (name, what)
    absent = (md == 0)[:, None, :].expand_as(k)
    for x in got[1:]:                                                    # absent columns: +0, not -0, not NaN
        assert not bool(x[absent].any()) and not bool(torch.signbit(x[absent]).any()), name
    for b in range(md.shape[0]):
        if not bool(md[b].any()):                                        # a keyless item: everything +0
            for x in got:
                assert not bool(x[b].any()) and not bool(torch.signbit(x[b]).any()), (name, b)


def _with_junk(k, v, md, junk):
    absent = (md == 0)[:, None, :].expand_as(k)
    return torch.where(absent, torch.full_like(k, junk), k), torch.where(absent, torch.full_like(v, junk), v)


# ------------------------------------------------------------------------------------------------------- 1. the chunk backward
CHUNK_SHAPES = [(3, 8, 128, 16, 16), (3, 8, 128, 1, 16), (2, 2, 8, 5, 32), (2, 2, 8, 3, 31)]


@pytest.mark.parametrize("B,H,dh,Tq,Tk", CHUNK_SHAPES)
def test_masked_chunk_backward_is_the_plain_kernel_on_compacted_keys(B, H, dh, Tq, Tk, dev):
    from multimodal_vqvae_compression_audio_tactile_amd import ops
    assert ops.attention_bwd_fits(dh, Tq, Tk)
    q, k, v, g = _qkvg(B, H * dh, Tq, Tk, B + H + dh + Tq + Tk, dev)
    plain = ops.attention_bwd(q, k, v, g, H)
    for name, mask in _masks(B, Tk, Tq + Tk).items():
        md, = _t(dev, mask)
        rc, *got = _chunk_raw(q, k, v, md, g, H)                          # outputs pre-filled with NaN: every element is written
        assert rc == 0, name
        want = _compacted_bwd(ops.attention_bwd, q, k, v, g, md, H)
        _check_against_compacted(got, want, md, k, name)
        for x, w in zip(ops.attention_bwd(q, k, v, g, H, kmask=md), got):  # the Python surface is that launch
            assert torch.equal(x, w), name
        if name == "all":
            for x, w in zip(got, plain):
                assert torch.equal(x, w)
        rc, *seq = _seq_raw(q, k, v, md, g, H)                            # the sequence form, wherever the chunk form fits
        assert rc == 0
        for x, w, what in zip(seq, got, ("gq", "gk", "gv")):
            assert torch.equal(x, w), (name, what, "seq vs chunk")
        if name in ("alternating", "per_item"):                           # an absent column never reaches any output
            for junk in (float("nan"), 1e30):
                k2, v2 = _with_junk(k, v, md, junk)
                for raw in (_chunk_raw, _seq_raw):
                    rc, *got2 = raw(q, k2, v2, md, g, H)
                    assert rc == 0
                    for x, w in zip(got2, want):
                        assert torch.equal(x, w), (name, junk, raw.__name__)
    rc, *raw = _chunk_raw(q, k, v, None, g, H)                            # a NULL mask is the existing launch
    assert rc == 0
    for x, w in zip(raw, plain):
        assert torch.equal(x, w)
    rc, *raw = _seq_raw(q, k, v, None, g, H)
    assert rc == 0
    for x, w in zip(raw, ops.attention_seq_bwd(q, k, v, g, H)):
        assert torch.equal(x, w)


def test_masked_chunk_backward_folded_layout_and_refusals(dev):
    """The layout of the training step, token-folded [1, C, B*n] with one mask row per item; a mask buffer with a row stride of its
    own; refused shapes return MVQ_EINVAL before any launch (the outputs keep their NaN)."""
    from multimodal_vqvae_compression_audio_tactile_amd import MvqError, _lib, ops
    B, H, dh, Tq, Tk = 3, 8, 128, 16, 11
    q, k, v, g = _qkvg(B, H * dh, Tq, Tk, 77, dev)
    mask = _masks(B, Tk, 5)["per_item"]
    md, = _t(dev, mask)
    want = ops.attention_bwd(q, k, v, g, H, kmask=md)
    got = ops.attention_bwd(fold(q), fold(k), fold(v), fold(g), H, folded_batch=B, kmask=md)
    for x, w in zip(got, want):
        assert torch.equal(unfold(x, B), w)
    wide = np.zeros((B, 20), np.uint8); wide[:, :Tk] = mask; wide[:, Tk:] = 1          # columns past Tk belong to no key
    wd, = _t(dev, wide)
    for x, w in zip(ops.attention_bwd(q, k, v, g, H, kmask=wd.reshape(-1), m_stride=20), want):
        assert torch.equal(x, w)
    fwd = ops.attention(fold(q), fold(k), fold(v), H, folded_batch=B, kmask=md)         # the forward of the same call
    assert torch.equal(unfold(fwd, B), ops.attention_seq(q, k, v, H, kmask=md))
    with pytest.raises(MvqError, match="mask row"):
        ops.attention_bwd(q, k, v, g, H, kmask=md.reshape(-1)[:-1].contiguous())
    with pytest.raises(MvqError, match="kmask"):
        ops.attention_bwd(q, k, v, g, H, kmask=md.bool())
    lib = _lib.lib()
    outs = [torch.full_like(x, float("nan")) for x in (q, k, v)]
    p = lambda x: x.data_ptr()
    for bad in ((B, H, dh, 33, Tk), (B, H, dh, Tq, 33), (B, 0, dh, Tq, Tk), (-1, H, dh, Tq, Tk), (B, 1, 256, 32, 32)):
        assert lib.mvq_attention_masked_bwd_f32(p(q), p(k), p(v), p(md), p(g), *(p(o) for o in outs), *bad, 0, 0, 0, 0, Tk,
                                                _stream()) == EINVAL, bad
    scratch = torch.empty(2 * B * H * 16 * 16, device=dev)
    for bad in ((B, H, dh, Tq, 513), (B, H, dh, 513, Tk), (B, 1, 257, Tq, Tk), (B, 0, dh, Tq, Tk)):   # Tk = 513: refused before launch
        assert lib.mvq_attention_seq_masked_bwd_f32(p(q), p(k), p(v), p(md), p(g), *(p(o) for o in outs), p(scratch), *bad, 0, 0, 0, 0, Tk,
                                                    _stream()) == EINVAL, bad
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(o).all()) for o in outs)


# ---------------------------------------------------------------------------------------------------- 2. the sequence backward
@pytest.mark.parametrize("B,H,dh,Tq,Tk", [(2, 8, 128, 75, 75), (1, 2, 8, 7, 130), (1, 2, 8, 4, 33)])
def test_masked_seq_backward_is_the_plain_kernels_on_compacted_keys(B, H, dh, Tq, Tk, dev):
    from multimodal_vqvae_compression_audio_tactile_amd import MvqError, ops
    q, k, v, g = _qkvg(B, H * dh, Tq, Tk, B + H + dh + Tq + Tk, dev)
    plain = ops.attention_seq_bwd(q, k, v, g, H)
    for name, mask in _seq_masks(B, Tk, Tq + Tk).items():
        md, = _t(dev, mask)
        rc, *got = _seq_raw(q, k, v, md, g, H)
        assert rc == 0, name
        want = _compacted_bwd(ops.attention_seq_bwd, q, k, v, g, md, H)
        _check_against_compacted(got, want, md, k, name)
        for x, w in zip(ops.attention_seq_bwd(q, k, v, g, H, kmask=md), got):
            assert torch.equal(x, w), name
        if name == "all":
            for x, w in zip(got, plain):
                assert torch.equal(x, w)
        if name in ("per_item", "tiles"):
            for junk in (float("nan"), 1e30):
                k2, v2 = _with_junk(k, v, md, junk)
                rc, *got2 = _seq_raw(q, k2, v2, md, g, H)
                assert rc == 0
                for x, w in zip(got2, want):
                    assert torch.equal(x, w), (name, junk)
    md, = _t(dev, _masks(B, Tk, 1)["per_item"])
    folded = ops.attention_seq_bwd(fold(q), fold(k), fold(v), fold(g), H, folded_batch=B, kmask=md)   # as the PLC step calls it
    for x, w in zip(folded, ops.attention_seq_bwd(q, k, v, g, H, kmask=md)):
        assert torch.equal(unfold(x, B), w)
    with pytest.raises(MvqError, match="kmask"):
        ops.attention_seq_bwd(q, k, v, g, H, kmask=md[:, :Tk - 1].contiguous())


# ------------------------------------------------------------------------------------------- 3. both forms against float64
@pytest.mark.parametrize("B,H,dh,Tq,Tk", [(3, 8, 128, 16, 16), (2, 8, 128, 75, 75)])
def test_masked_backward_against_float64_autograd(B, H, dh, Tq, Tk, dev):
    from multimodal_vqvae_compression_audio_tactile_amd import ops
    gen = torch.Generator().manual_seed(B * 1000 + Tk)
    q, k, v, go = (torch.randn(B, H * dh, t, generator=gen, dtype=torch.float64) for t in (Tq, Tk, Tk, Tq))
    mask = torch.from_numpy(_masks(B, Tk, 9)["per_item"])
    qr, kr, vr = (x.clone().requires_grad_(True) for x in (q, k, v))
    sp = lambda x: x.reshape(B, H, dh, -1).permute(0, 1, 3, 2)
    ctx = lt.masked_attention(sp(qr), sp(kr), sp(vr), mask != 0, dh).permute(0, 1, 3, 2).reshape(B, H * dh, Tq)
    (ctx * go).sum().backward()
    args = [x.float().to(dev) for x in (q, k, v, go)]
    forms = {"seq": ops.attention_seq_bwd(*args, H, kmask=mask.to(dev))}
    if ops.attention_bwd_fits(dh, Tq, Tk):
        forms["chunk"] = ops.attention_bwd(*args, H, kmask=mask.to(dev))
    for form, got in forms.items():
        for name, gt, want in zip(("gq", "gk", "gv"), got, (qr.grad, kr.grad, vr.grad)):
            assert torch.isfinite(gt).all(), (form, name)
            r = rel(gt, want)
            print(f"masked attention bwd {form} B={B} T={Tk} {name}: rel L2 {r:.2e}")
            assert r <= TOL, (form, name, r)


# ------------------------------------------------------------------------------------------------------------ 4. the loss draw
DRAW_CHANNELS = {"iid": packets.Channel(loss=0.3, thin=0.4, min_books=1, seed=3),
                 "burst": packets.Channel(loss=0.05, thin=0.4, min_books=2, p_gb=0.15, p_bg=0.35, loss_bad=0.9, seed=11)}


@pytest.mark.parametrize("nb,T,ptok,B", [(8, 75, 2, 3), (32, 37, 2, 2), (9, 5, 1, 1), (10, 16, 16, 4)])
def test_channel_draw_equals_the_numpy_definition(nb, T, ptok, B, dev):
    from multimodal_vqvae_compression_audio_tactile_amd import ops
    P = (T + ptok - 1) // ptok
    for name, ch in DRAW_CHANNELS.items():
        for base in (0, 4000000000):
            for stream, step in ((0, 0), (1, 7)):
                got = ops.channel_draw(ch, nb, T, ptok, B, stream=stream, step=step, item_base=base, device=dev)
                want = np.repeat(packets.channel_counts(ch, nb, P, B, stream=stream, step=step, item_base=base), ptok, axis=1)[:, :T]
                assert got.dtype == torch.uint8 and tuple(got.shape) == (B, T)
                assert np.array_equal(got.cpu().numpy(), want), (name, base, stream, step)
    big = ops.channel_draw(DRAW_CHANNELS["burst"], nb, T, ptok, 256, step=2, device=dev)        # more than one block; batch invariance
    small = ops.channel_draw(DRAW_CHANNELS["burst"], nb, T, ptok, 6, step=2, device=dev)
    assert torch.equal(big[:6], small)
    assert np.array_equal(big.cpu().numpy(), np.repeat(packets.channel_counts(DRAW_CHANNELS["burst"], nb, P, 256, step=2), ptok, axis=1)[:, :T])


# ------------------------------------------------------------------------------------------------------------ 5. the whole step
def _loss(out, wy):
    y, tgt = out["y_hat"], out["tgt"]
    return (y - tgt).abs().mean() + (y * wy[..., :y.shape[-1]]).mean()


def _step_case():
    """B = 2, 24 tokens = two AR chunks.  The explicit masks: a lost packet holding the LAST token of chunk 0 (its z_hat, the
    prediction alone, feeds chunk 1), a lost first packet, packets thinned to 1 and 2 books, lost audio tokens (the first packet of
    an item among them: "hold" has nothing to hold yet), and chunk 1 of item 1 without any audio key."""
    if "case" not in _CACHE:
        from multimodal_vqvae_compression_audio_tactile_amd import synth
        sd = synth.proposed_model_state(23, rvq_books=3, rvq_embed=128)
        T = 320 * 24
        a = synth.audio_segments(2, seed=9, T=T); t = synth.tactile_segments(2, seed=9, T=T)
        wy = 0.05 * torch.randn(2, 1, T, generator=torch.Generator().manual_seed(4))
        nbv = torch.full((2, 24), 3, dtype=torch.uint8)
        nbv[0, 14:16] = 0; nbv[1, 0:2] = 0; nbv[0, 4:6] = 1; nbv[1, 18:20] = 2; nbv[0, 20:22] = 0
        nav = torch.full((2, 24), 32, dtype=torch.uint8)
        nav[0, 2:4] = 0; nav[0, 10] = 0; nav[0, 17] = 0; nav[0, 6] = 5
        nav[1, 0:2] = 0; nav[1, 12:14] = 0; nav[1, 16:24] = 0
        ref = O.ProposedEval(rvq_books=3, rvq_embed=128)
        ref.load_state_dict({k: v for k, v in sd.items() if k != "predict.pos.pe"}, strict=False)
        ref.eval()
        for m in (ref.A_ENC, ref.A_QUANT, ref.T_ENC, ref.T_DEC):
            for p in m.parameters():
                p.requires_grad_(False)
        _CACHE["case"] = (sd, a, t, wy, nbv, nav, ref)
    return _CACHE["case"]


@torch.enable_grad()
@pytest.mark.parametrize("mode", ["zero", "mask", "hold"])
def test_allpredar_link_training_step(mode, dev):
    """(a) the recorded forward is the no_grad forward; (b) decode_latents on what the step says it transmitted reproduces its
    z_run exactly: every op of the loop is the receiver's; (c) the indices are the restatement's; (d) all 21 trainable tensors
    within TOL of the restatement's autograd; (e) vq.books and the frozen backbones get no gradient; (f) r_tokens covers every
    token and every book: equal to the restatement's rD, and -- with na_valid = None -- bit-equal to the default step's over
    chunk 0.  (Beyond chunk 0 the closed loop feeds the receiver's z_hat, not the lossless one, into the predictor, so rD itself
    differs from the default step's there: no equality exists to assert.)"""
    from multimodal_vqvae_compression_audio_tactile_amd import AllPredAR, build_proposed
    sd, a, t, wy, nbv, nav, ref = _step_case()
    ref.zero_grad(set_to_none=True)
    out_r = lt.forward_step_link(ref, a, t, nbv, nav, mode)
    _loss(out_r, wy).backward()

    net = build_proposed(sd, rvq_books=3, rvq_embed=128, device=dev, cls=AllPredAR)       # .eval(): dropout off
    ad, td, nbd, nad = a.to(dev), t.to(dev), nbv.to(dev), nav.to(dev)
    out = net.forward_step(ad, td, nb_valid=nbd, na_valid=nad, audio_conceal=mode)
    with torch.no_grad():
        out_inf = net.forward_step(ad, td, nb_valid=nbd, na_valid=nad, audio_conceal=mode)
        rx = net.decode_latents(out["codes"], out["idx"], nb_valid=nbd, na_valid=nad, audio_conceal=mode)
    for key in ("y_hat", "z_run", "idx", "r_tokens"):                                     # (a)
        assert torch.equal(out[key], out_inf[key]), key
    assert torch.equal(rx, out["z_run"].detach())                                         # (b)
    assert torch.equal(out["idx"].cpu(), out_r["idx"])                                    # (c)
    assert torch.equal(out["codes"].cpu(), out_r["codes"])
    assert torch.equal(out["nb_valid"], nbd) and torch.equal(out["na_valid"], nad)
    assert rel(out["z_run"], out_r["z_run"]) < 1e-3 and rel(out["y_hat"], out_r["y_hat"]) < 1e-3
    assert tuple(out["r_tokens"].shape) == (2, 96, 24) and rel(out["r_tokens"], out_r["r_tokens"]) < 1e-3   # (f)
    _loss(out, wy.to(dev)).backward()
    named_r = dict(ref.named_parameters())
    checked, worst = 0, 0.0
    for name, p in net.named_parameters():
        if name.startswith("vq.books") or name.split(".")[0] in ("A_ENC", "A_QUANT", "T_ENC", "T_DEC"):
            assert p.grad is None, name                                                    # (e)
            continue
        assert p.grad is not None, name
        want = named_r[name].grad
        assert float(want.norm()) > 0, name
        err = rel(p.grad, want)
        print(f"  [{mode}] {name:28s} |g| {float(want.norm()):.3e}  rel err {err:.2e}")
        worst = max(worst, err)
        assert err < TOL, (name, err)                                                      # (d)
        checked += 1
    assert checked == 21
    print(f"[{mode}] worst relative gradient error over {checked} tensors: {worst:.2e}")


def test_allpredar_link_step_defaults_link_and_rtokens(dev):
    from multimodal_vqvae_compression_audio_tactile_amd import AllPredAR, build_proposed, ops
    sd, a, t, wy, nbv, nav, ref = _step_case()
    net = build_proposed(sd, rvq_books=3, rvq_embed=128, device=dev, cls=AllPredAR)
    ad, td, nbd = a.to(dev), t.to(dev), nbv.to(dev)
    with torch.no_grad():
        base = net._forward_step(ad, td)[0]                               # the parent's body
        dflt = net.forward_step(ad, td)
        kw = net.forward_step(ad, td, nb_valid=None, na_valid=None, audio_conceal="zero", link=None, step=5)
        assert set(dflt) == set(base) == {"y_hat", "tgt", "r_tokens"}
        for key in base:
            assert torch.equal(dflt[key], base[key]) and torch.equal(kw[key], base[key]), key
        lossy = net.forward_step(ad, td, nb_valid=nbd)                    # na_valid = None: the straight-through qa of the default step
        assert lossy["na_valid"] is None and torch.equal(lossy["r_tokens"][..., :16], base["r_tokens"][..., :16])
        assert not torch.equal(lossy["y_hat"], base["y_hat"])
        full = net.forward_step(ad, td, nb_valid=torch.full_like(nbd, 3))  # nothing lost: the default step, round-off apart
        d = rel(full["y_hat"], base["y_hat"])
        print(f"link step with nothing lost vs the default step: relative L2 of y_hat {d:.2e}")
        assert d < 1e-3
        # link= / step=: the masks are ops.channel_draw's, stream 0 tactile (3 books) and stream 1 audio (32 stages)
        link = packets.Link(packets.Channel(loss=0.2, thin=0.3, seed=5), packets.Channel(loss=0.2, p_gb=0.2, p_bg=0.5, seed=6), 2)
        o3 = net.forward_step(ad, td, link=link, step=3, audio_conceal="mask")
        o4 = net.forward_step(ad, td, link=link, step=4, audio_conceal="mask")
        assert torch.equal(o3["nb_valid"], ops.channel_draw(link.tactile, 3, 24, 2, 2, stream=0, step=3, device=dev))
        assert torch.equal(o3["na_valid"], ops.channel_draw(link.audio, 32, 24, 2, 2, stream=1, step=3, device=dev))
        assert not torch.equal(o3["nb_valid"], o4["nb_valid"]) and not torch.equal(o3["na_valid"], o4["na_valid"])
        assert bool((o3["nb_valid"] == 0).any()) and bool((o3["na_valid"] == 0).any())
        rx = net.decode_latents(o3["codes"], o3["idx"], nb_valid=o3["nb_valid"], na_valid=o3["na_valid"], audio_conceal="mask")
        assert torch.equal(rx, o3["z_run"])
        o_t = net.forward_step(ad, td, link=packets.Link(link.tactile), step=3)           # tactile loss alone
        assert o_t["na_valid"] is None and torch.equal(o_t["nb_valid"], o3["nb_valid"])
    with torch.enable_grad():                                             # a link step records and trains
        o = net.forward_step(ad, td, link=link, step=3, audio_conceal="hold")
        _loss(o, wy.to(dev)).backward()
        assert all(torch.isfinite(p.grad).all() for n, p in net.named_parameters() if p.grad is not None)
        assert net.predict.q_proj.weight.grad is not None and net.vq.books[0].grad is None


# ----------------------------------------------------------------------------------------------------------------- 6. the PLC step
@torch.enable_grad()
@pytest.mark.parametrize("mode", ["mask", "hold"])
def test_allpredplc_link_training_step(mode, dev):
    """T_lat = 75: the predictor runs ONCE over the sequence, on the masked full-sequence attention and its backward."""
    from multimodal_vqvae_compression_audio_tactile_amd import build_plc, ops, synth
    sd, _, _, _, _, _, ref = _step_case()
    B, T = 2, 24000
    a = synth.audio_segments(B, seed=12, T=T); t = synth.tactile_segments(B, seed=12, T=T)
    wy = 0.05 * torch.randn(B, 1, T, generator=torch.Generator().manual_seed(6))
    r = np.random.default_rng(8)
    lost = torch.from_numpy(np.repeat(r.uniform(size=(B, 38)) < 0.5, 2, axis=1)[:, :75].copy())
    nav = torch.from_numpy(np.repeat(np.where(r.uniform(size=(B, 38)) < 0.4, 0, 32).astype(np.uint8), 2, axis=1)[:, :75].copy())
    nav[0, 0:2] = 0; nav[1, 0:2] = 32; nav[1, 40] = 7
    ref.zero_grad(set_to_none=True)
    out_r = lt.plc_step_link(ref, a, t, lost, nav, mode)
    _loss(out_r, wy).backward()

    net = build_plc(device=dev)
    missing, unexpected = net.load_state_dict({k: v for k, v in sd.items() if k.split(".")[0] in ("A_ENC", "A_QUANT", "T_ENC", "T_DEC", "predict", "tokennorm")},
                                              strict=False)
    assert not missing and not unexpected
    ad, td, ld, nd = a.to(dev), t.to(dev), lost.to(dev), nav.to(dev)
    out = net.forward_step(ad, td, mask=ld, na_valid=nd, audio_conceal=mode)
    with torch.no_grad():
        out_inf = net.forward_step(ad, td, mask=ld, na_valid=nd, audio_conceal=mode)
    assert torch.equal(out["y_hat"], out_inf["y_hat"]) and torch.equal(out["latent_mask"][:, 0], ld)
    assert rel(out["y_hat"], out_r["y_hat"]) < 1e-3
    _loss(out, wy.to(dev)).backward()
    named_r = dict(ref.named_parameters())
    checked = 0
    for name, p in net.named_parameters():
        if not name.startswith("predict.") or not p.requires_grad:
            assert p.grad is None, name
            continue
        err = rel(p.grad, named_r[name].grad)
        print(f"  [plc {mode}] {name:28s} rel err {err:.2e}")
        assert float(named_r[name].grad.norm()) > 0 and err < TOL, (name, err)
        checked += 1
    assert checked == 14
    if mode == "mask":                                                    # NaN in absent audio columns of a hand-built qa
        with torch.no_grad():
            zt = net.T_ENC(td)
            qa = ops._dev(net.A_QUANT.from_codes(out["codes"], nq_valid=nd)[0], "qa")
            zt_in, _ = ops.plc_mask_fill(zt, None, ld)
            bad = torch.where((nd == 0)[:, None, :].expand_as(qa), torch.full_like(qa, float("nan")), qa)
            clean = net._fill_decode(zt, zt_in, qa, ld, nd)
            assert torch.equal(net._fill_decode(zt, zt_in, bad, ld, nd), clean) and bool(torch.isfinite(clean).all())
        with torch.enable_grad():
            assert torch.equal(net._fill_decode(zt, zt_in, bad, ld, nd).detach(), clean)
