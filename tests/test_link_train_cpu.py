"""CPU: the loss-pattern definition (packets.channel_counts), the torch restatement of the link training step
(tests/link_train_oracle.py) and every refusal of the two forward_steps that happens before a launch."""
import math

import numpy as np
import pytest
import torch

import link_train_oracle as lt
from multimodal_vqvae_compression_audio_tactile_amd import packets
from multimodal_vqvae_compression_audio_tactile_amd.packets import Channel, Link, channel_counts

O = lt.O


# ------------------------------------------------------------------------------------------------------ 1. channel_counts
def _scalar_counts(ch, nb, P, items, stream=0, step=0, item_base=0):
    """The docstring of channel_counts read literally, one Python int at a time."""
    M = 0xFFFFFFFF

    def mix(x):
        x ^= x >> 16; x = (x * 0x7feb352d) & M; x ^= x >> 15; x = (x * 0x846ca68b) & M
        return x ^ (x >> 16)

    fold = lambda h, f: mix(((h ^ (f & M)) + 0x9e3779b9) & M)
    t_loss, t_thin, t_gb, t_bg, t_lbad = ch.thresholds()
    hs = fold(fold(fold(0, ch.seed), step), stream)
    out = np.zeros((items, P), np.uint8)
    for b in range(items):
        hi, bad = fold(hs, item_base + b), False
        for p in range(P):
            h = fold(hi, p)
            u0 = fold(h, 0)
            bad = (not u0 < t_bg) if bad else (u0 < t_gb)
            c = nb
            if fold(h, 1) < (t_lbad if bad else t_loss):
                c = 0
            elif nb > ch.min_books and fold(h, 2) < t_thin:
                c = ch.min_books + ((fold(h, 3) * (nb - ch.min_books)) >> 32)
            out[b, p] = c
    return out


BURST = Channel(loss=0.05, thin=0.4, min_books=2, p_gb=0.15, p_bg=0.35, loss_bad=0.9, seed=11)
IID = Channel(loss=0.3, thin=0.3, min_books=1, seed=3)


def test_channel_counts_definition_and_invariants():
    for ch in (BURST, IID):
        a = channel_counts(ch, 8, 40, 256, stream=1, step=5)
        assert a.dtype == np.uint8 and a.shape == (256, 40)
        assert np.array_equal(a, channel_counts(ch, 8, 40, 256, stream=1, step=5))              # same arguments, same array
        assert np.array_equal(a[:6], channel_counts(ch, 8, 40, 6, stream=1, step=5))            # rows 0..5 of 256 are the 6
        assert np.array_equal(a[100:106], channel_counts(ch, 8, 40, 6, stream=1, step=5, item_base=100))
        assert np.array_equal(a[:9], _scalar_counts(ch, 8, 40, 9, stream=1, step=5))
        assert 0 < (a == 0).mean() < 1 and ((a > 0) & (a < 8)).any()
        for other in (channel_counts(ch, 8, 40, 256, stream=0, step=5), channel_counts(ch, 8, 40, 256, stream=1, step=6),
                      channel_counts(dataclass_replace(ch, seed=ch.seed + 1), 8, 40, 256, stream=1, step=5)):
            assert not np.array_equal(a, other)
    assert np.array_equal(channel_counts(Channel(), 8, 17, 5), np.full((5, 17), 8, np.uint8))      # loss = 0, thin = 0: all nb
    assert not channel_counts(Channel(loss=1.0), 8, 17, 5).any()                                   # loss = 1: all lost
    assert not channel_counts(Channel(p_gb=1.0, p_bg=0.0, loss_bad=1.0), 8, 17, 5).any()           # bad from packet 0 on
    t = channel_counts(Channel(thin=1.0, min_books=3), 8, 200, 8)
    assert t.min() == 3 and t.max() == 7                                                           # every count in 3..7
    assert np.array_equal(channel_counts(Channel(thin=1.0, min_books=8), 8, 30, 4), np.full((4, 30), 8, np.uint8))
    # the burst channel loses in runs: longer mean run than the i.i.d. channel of the same loss rate
    b = channel_counts(Channel(p_gb=0.05, p_bg=0.2, seed=1), 8, 4000, 4) == 0
    i = channel_counts(Channel(loss=float(b.mean()), seed=1), 8, 4000, 4) == 0
    runs = lambda m: m.sum() / max(1, (np.diff(m.astype(np.int8), axis=1) == 1).sum() + m[:, 0].sum())
    assert runs(b) > 2 * runs(i)
    with pytest.raises(ValueError, match="bad shape"):
        channel_counts(Channel(min_books=9), 8, 4, 1)


def dataclass_replace(ch, **kw):
    import dataclasses
    return dataclasses.replace(ch, **kw)


def test_channel_and_link_refuse_bad_values():
    for name in ("loss", "thin", "p_gb", "p_bg", "loss_bad"):
        for bad in (-0.01, 1.01, float("nan"), "0.5"):
            with pytest.raises(ValueError, match=name):
                Channel(**{name: bad})
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError, match="min_books"):
            Channel(min_books=bad)
    with pytest.raises(ValueError, match="Link"):
        Link(tactile=None)
    with pytest.raises(ValueError, match="Link"):
        Link(Channel(), audio=0.5)
    with pytest.raises(ValueError, match="packet_tok"):
        Link(Channel(), packet_tok=0)
    assert Channel(loss=1.0).thresholds()[0] == 1 << 32 and Channel(loss=0.5).thresholds()[0] == 1 << 31
    assert Link(Channel(), Channel(), 4).packet_tok == 4


# -------------------------------------------------------------------------------------------------------------- 2. the oracle
def _split(x, H):
    B, C, T = x.shape
    return x.permute(0, 2, 1).reshape(B, T, H, C // H).permute(0, 2, 1, 3)


def test_oracle_masked_attention():
    g = torch.Generator().manual_seed(2)
    B, H, dh, Tq, Tk = 3, 2, 8, 5, 9
    Q, K, V = (torch.randn(B, H, t, dh, generator=g, dtype=torch.float64).requires_grad_(True) for t in (Tq, Tk, Tk))
    plain = ((Q @ K.transpose(-2, -1)) / math.sqrt(dh)).softmax(-1) @ V
    assert torch.equal(lt.masked_attention(Q, K, V, torch.ones(B, Tk, dtype=torch.bool), dh), plain)   # all present: exactly
    mask = torch.rand(B, Tk, generator=g) < 0.5
    mask[0, 0], mask[1, 0] = False, True
    mask[2] = False                                                                                    # a keyless item
    ctx = lt.masked_attention(Q, K, V, mask, dh)
    (ctx * torch.randn(ctx.shape, generator=g, dtype=torch.float64)).sum().backward()
    absent = ~mask[:, None, :, None].expand_as(K)
    assert not bool(K.grad[absent].any()) and not bool(V.grad[absent].any())                           # exactly 0
    assert bool(K.grad[~absent].any()) and bool(V.grad[~absent].any())
    assert not bool(ctx[2].any()) and not bool(Q.grad[2].any()) and bool(torch.isfinite(Q.grad).all())
    for b in range(2):                                                                                 # = the compacted call
        J = torch.nonzero(mask[b]).reshape(-1)
        want = ((Q[b] @ K[b][:, J].transpose(-2, -1)) / math.sqrt(dh)).softmax(-1) @ V[b][:, J]
        assert torch.allclose(ctx[b], want, rtol=0, atol=1e-14)
    # NaN in an absent column changes nothing
    K2, V2 = K.detach().clone(), V.detach().clone()
    K2[absent], V2[absent] = float("nan"), float("nan")
    assert torch.equal(lt.masked_attention(Q.detach(), K2, V2, mask, dh), ctx.detach())


def test_oracle_predictor_and_layered_ste():
    torch.manual_seed(5)
    pr = O.CrossPredictor(64, heads=4).eval()
    zt_prev, za = torch.randn(2, 64, 7), torch.randn(2, 64, 7)
    assert torch.equal(lt.predictor(pr, zt_prev, za, torch.full((2, 7), 3, dtype=torch.uint8)), pr(zt_prev, za))
    assert torch.equal(lt.predictor(pr, zt_prev, za, None), pr(zt_prev, za))
    vq = O.ResidualVQEMA(12, 3, 16)
    rD = torch.randn(2, 12, 6).requires_grad_(True)
    nbv = torch.tensor([[3, 0, 1, 2, 3, 0], [0, 3, 3, 1, 2, 2]], dtype=torch.uint8)
    q, idx = lt.layered_ste(vq, rD, nbv)
    g = torch.randn(q.shape)
    (q * g).sum().backward()
    assert torch.equal(rD.grad, g * nbv.unsqueeze(1).float())                  # m * g per token; a lost token gets exactly 0
    assert not bool(rD.grad[:, :, :][nbv.unsqueeze(1).expand_as(g) == 0].any())
    assert all(p.grad is None for p in vq.books)
    want = torch.zeros_like(q)                                                 # the receiver's sum: book order, from +0
    for i, cb in enumerate(vq.books):
        want = want + (nbv.unsqueeze(1) > i).float() * cb.detach()[idx[i]].permute(0, 2, 1)
    assert torch.equal(q.detach(), want) and not bool(q[0, :, 1].any())
    full, idx_full = lt.layered_ste(vq, rD.detach(), torch.full((2, 6), 3))
    assert torch.equal(idx_full, idx)                                          # the search does not depend on the counts
    assert torch.allclose(full, vq(rD.detach()), rtol=0, atol=1e-6)            # the straight-through sum: round-off apart
    qa = torch.arange(24, dtype=torch.float32).reshape(1, 2, 12)
    nav = torch.tensor([[0, 0, 1, 0, 0, 5, 0, 1, 1, 0, 0, 0]], dtype=torch.uint8)
    h = lt.hold_fill(qa, nav)
    assert torch.equal(h[0, 0], torch.tensor([0., 0, 2, 2, 2, 5, 5, 7, 8, 8, 8, 8]))


# ------------------------------------------------------------------------------------------------------------- 3. refusals
def test_forward_steps_refuse_before_any_launch():
    """On nets built on the CPU: a launch would fail with another error, so each message proves the refusal came first."""
    from multimodal_vqvae_compression_audio_tactile_amd import AllPredAR, MvqError, build_plc, build_proposed
    from multimodal_vqvae_compression_audio_tactile_amd.proposed import encoder_out_len
    net = build_proposed(None, rvq_books=2, rvq_embed=128, device="cpu", cls=AllPredAR)
    plc = build_plc(device="cpu")
    T = 320 * 24
    a, t = torch.zeros(2, 1, T), torch.zeros(2, 1, T)
    assert encoder_out_len(net.T_ENC, T) == 24 and encoder_out_len(net.T_ENC, 24000) == 75 and encoder_out_len(net.T_ENC, 1) == 0
    assert encoder_out_len(torch.nn.Identity(), T) is None
    ok = torch.full((2, 24), 2, dtype=torch.uint8)
    link = Link(Channel(loss=0.1), Channel(loss=0.1), 2)
    for kw, msg in (
        ({"nb_valid": ok.bool()}, "nb_valid must be a uint8"),
        ({"nb_valid": ok.float()}, "nb_valid must be a uint8"),
        ({"nb_valid": [[1] * 24] * 2}, "nb_valid must be a uint8"),
        ({"nb_valid": ok[:, :23]}, "nb_valid .* does not match"),
        ({"nb_valid": ok[:1]}, "nb_valid .* does not match"),
        ({"nb_valid": ok.reshape(2, 1, 24)}, "nb_valid .* does not match"),
        ({"na_valid": ok.int()}, "na_valid must be a uint8"),
        ({"na_valid": ok[:, :5]}, "na_valid .* does not match"),
        ({"audio_conceal": "repeat"}, "audio_conceal must be"),
        ({"audio_conceal": "repeat", "na_valid": ok}, "audio_conceal must be"),
        ({"link": link, "nb_valid": ok}, "link draws the masks itself"),
        ({"link": link, "na_valid": ok}, "link draws the masks itself"),
        ({"link": (Channel(), None, 2)}, "link must be a packets.Link"),
        ({"audio_conceal": "mask"}, "needs na_valid or a link"),
        ({"audio_conceal": "hold", "nb_valid": ok}, "needs na_valid or a link"),
        ({"audio_conceal": "hold", "link": Link(Channel(loss=0.1))}, "needs na_valid or a link"),
    ):
        with pytest.raises(MvqError, match=msg):
            net.forward_step(a, t, **kw)
    for kw, msg in (
        ({"na_valid": ok.bool()}, "na_valid must be a uint8"),
        ({"na_valid": ok[:, :23]}, "na_valid .* does not match"),
        ({"na_valid": ok, "audio_conceal": "repeat"}, "audio_conceal must be"),
        ({"audio_conceal": "mask"}, "needs na_valid"),
        ({"audio_conceal": "hold"}, "needs na_valid"),
    ):
        with pytest.raises(MvqError, match=msg):
            plc.forward_step(a, t, **kw)
    # the predictor's forward keeps refusing a key mask under autograd: the training entry points call run_train themselves
    zt, za = torch.zeros(1, 1024, 4), torch.zeros(1, 1024, 4)
    with torch.enable_grad():
        with pytest.raises(MvqError, match="inference only"):
            net.predict(zt, za, key_mask=torch.ones(1, 4, dtype=torch.uint8))
        with pytest.raises(MvqError, match="inference only"):
            plc.predict(zt, za, key_mask=torch.ones(1, 4, dtype=torch.uint8))


def test_ops_refuse_host_tensors_and_bad_draws():
    from multimodal_vqvae_compression_audio_tactile_amd import MvqError, ops
    with pytest.raises(MvqError, match="packets.Channel"):
        ops.channel_draw(None, 8, 10, 2, 3)
    with pytest.raises(MvqError, match="bad shape"):
        ops.channel_draw(Channel(min_books=9), 8, 10, 2, 3)
    with pytest.raises(MvqError, match="bad shape"):
        ops.channel_draw(Channel(), 8, 10, 0, 3)
    q = torch.zeros(1, 16, 4)
    for fn in (lambda: ops.attention(q, q, q, 2, kmask=torch.ones(1, 4, dtype=torch.uint8)),
               lambda: ops.attention_bwd(q, q, q, q, 2, kmask=torch.ones(1, 4, dtype=torch.uint8)),
               lambda: ops.attention_seq_bwd(q, q, q, q, 2, kmask=torch.ones(1, 4, dtype=torch.uint8))):
        with pytest.raises(MvqError):
            fn()


def test_new_symbols_are_exported_and_refuse_bad_shapes():
    from multimodal_vqvae_compression_audio_tactile_amd import _lib
    lib = _lib.lib()
    assert lib.mvq_abi_version() == 3
    junk = 64                                                                  # never dereferenced: every call is refused first
    for bad in ((1, 1, 8, 33, 8), (1, 1, 8, 8, 33), (1, 0, 8, 8, 8), (-1, 1, 8, 8, 8), (1, 1, 256, 32, 32)):
        assert lib.mvq_attention_masked_bwd_f32(junk, junk, junk, junk, junk, junk, junk, junk, *bad, 0, 0, 0, 0, 8, None) == -1, bad
    for bad in ((1, 1, 8, 8, 513), (1, 1, 8, 513, 8), (1, 1, 257, 8, 8), (1, 0, 8, 8, 8)):
        assert lib.mvq_attention_seq_masked_bwd_f32(junk, junk, junk, junk, junk, junk, junk, junk, junk, *bad, 0, 0, 0, 0, 8, None) == -1, bad
    one = 1 << 32
    for bad in ((1, 4, 0, 8, 1), (1, 4, 2, 8, 9), (1, 4, 2, 0, 1), (1, 4, 2, 256, 1), (1, 4, 2, 8, 0), (-1, 4, 2, 8, 1)):
        assert lib.mvq_channel_draw_u8(junk, *bad, 0, 0, 0, one, one, 0, 0, 0, 0, None) == -1, bad
    assert lib.mvq_channel_draw_u8(junk, 1, 4, 2, 8, 1, one + 1, 0, 0, one, one, 0, 0, 0, 0, None) == -1
    assert lib.mvq_channel_draw_u8(None, 0, 4, 2, 8, 1, 0, 0, 0, one, one, 0, 0, 0, 0, None) == 0      # nothing to draw
