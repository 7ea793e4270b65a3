"""-m gpu: the whole-stack C entry points (include/mvq.h "whole stacks": mvq_encoder_fwd_f32, mvq_decoder_fwd_f32,
mvq_decoder_fwd_saving_f32, mvq_decoder_bwd_input_f32) through ctypes -- bit-equal to the per-layer plan walked from Python (the
module path of rounds 1-4, kept as Encoder.forward_plan / Decoder.forward_plan) and to the C oracle, from one segment to the
headline batch."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _models(dev, seed=7):
    import multimodal_vqvae_compression_audio_tactile_amd as mvq
    from multimodal_vqvae_compression_audio_tactile_amd import synth
    sd = synth.dac_state(seed)
    mdl = mvq.DAC(); mdl.load_state_dict(sd, strict=True)
    return mdl.to(dev).eval(), sd


@pytest.mark.parametrize("B", [1, 48, 256])
def test_stacks_equal_the_per_layer_plan(B, dev):
    """B = 1: latency tiles; 48: the packed / virtually packed latent-rate rows (>= 32); 256: the headline batch."""
    from multimodal_vqvae_compression_audio_tactile_amd import dac, synth
    mdl, _ = _models(dev)
    x = synth.tactile_segments(B, seed=3).to(dev)
    assert dac.USE_STACKS
    z = mdl.encoder(x)                                               # mvq_encoder_fwd_f32
    z_plan = mdl.encoder.forward_plan(x)
    assert z.shape == z_plan.shape == (B, 1024, 75) and torch.equal(z, z_plan)
    del z_plan
    y = mdl.decoder(z)                                               # mvq_decoder_fwd_f32
    y_plan = mdl.decoder.forward_plan(z)
    assert y.shape == y_plan.shape == (B, 1, 23992) and torch.equal(y, y_plan)


def test_stacks_equal_the_oracle(orc, dev):
    from multimodal_vqvae_compression_audio_tactile_amd import synth
    mdl, sd = _models(dev)
    sdn = {k: v.numpy() for k, v in sd.items()}
    T = 320 * 18
    x = synth.audio_segments(2, seed=5, T=T)
    z = mdl.encoder(x.to(dev))
    want_z = orc.dac_encoder({k[len("encoder."):]: v for k, v in sdn.items() if k.startswith("encoder.")}, x.numpy())
    assert np.array_equal(z.cpu().numpy(), want_z)
    y = mdl.decoder(z)
    want_y = orc.dac_decoder({k[len("decoder."):]: v for k, v in sdn.items() if k.startswith("decoder.")}, want_z)
    assert np.array_equal(y.cpu().numpy(), want_y)
    # ragged lengths: not a multiple of the hop, shorter than a token, empty batch
    for T2, B2 in ((320 * 20 + 137, 2), (100, 2), (24000, 0)):
        x2 = synth.tactile_segments(max(B2, 1), seed=6, T=T2)[:B2].to(dev)
        z2 = mdl.encoder(x2)
        assert torch.equal(z2, mdl.encoder.forward_plan(x2))
        y2 = mdl.decoder(z2)
        assert y2.shape == (B2, 1, mdl.decoder.stack().out_len(z2.shape[-1]))
        if z2.shape[-1]:
            assert torch.equal(y2, mdl.decoder.forward_plan(z2))


@pytest.mark.parametrize("B", [1, 6])
def test_decoder_backward_through_the_stack(B, dev):
    """mvq_decoder_fwd_saving_f32 + mvq_decoder_bwd_input_f32 == the per-layer saving forward / input-gradient of the Python plan
    (itself bit-exact against the oracle: test_decoder_input_gradient_bit_exact), through autograd as the training step uses it."""
    from multimodal_vqvae_compression_audio_tactile_amd import dac
    mdl, _ = _models(dev)
    dec = mdl.decoder
    for p in dec.parameters():
        p.requires_grad_(False)
    g = torch.Generator().manual_seed(B)
    z0 = torch.randn(B, 1024, 24, generator=g).to(dev)
    gy = torch.randn(B, 1, dec.stack().out_len(24), generator=g).to(dev)

    def run():
        z = z0.clone().requires_grad_(True)
        y = dec(z)
        y.backward(gy)
        return y.detach(), z.grad
    y1, g1 = run()
    dac.USE_STACKS = False
    try:
        y2, g2 = run()
    finally:
        dac.USE_STACKS = True
    assert torch.equal(y1, y2) and torch.equal(g1, g2)
    assert torch.equal(y1, dec(z0))                                  # the saving forward computes the inference values


def test_stack_calls_are_capturable_and_registered_as_operators(dev):
    import multimodal_vqvae_compression_audio_tactile_amd.torch_ops  # noqa: F401
    from multimodal_vqvae_compression_audio_tactile_amd import synth
    from multimodal_vqvae_compression_audio_tactile_amd.graphs import GraphedCall
    mdl, _ = _models(dev)
    x = synth.tactile_segments(2, seed=9, T=320 * 30).to(dev)
    z = mdl.encoder(x); y = mdl.decoder(z)
    o = torch.ops.mi355x_vqvae
    assert torch.equal(o.encoder_fwd(x, mdl.encoder.stack().id), z)
    assert torch.equal(o.decoder_fwd(z, mdl.decoder.stack().id), y)
    gy = torch.ones_like(y)
    zz = z.clone().requires_grad_(True)
    for p in mdl.decoder.parameters():
        p.requires_grad_(False)
    mdl.decoder(zz).backward(gy)
    assert torch.equal(o.decoder_bwd_input(z, gy, mdl.decoder.stack().id), zz.grad)
    g = GraphedCall(lambda xx: mdl.decoder(mdl.encoder(xx)), x)      # no allocation / synchronisation inside the C calls
    assert torch.equal(g(x), y)


def test_encoder_stack_falls_back_without_the_dma_form(dev):
    """at B >= 32 the virtually packed tail needs the LDS-DMA ring; where the library has no such form for a shape it
    answers MVQ_EUNSUPPORTED and both the stack and the Python plan take the plain launches (same results)."""
    from multimodal_vqvae_compression_audio_tactile_amd import dac, ops
    enc = dac.Encoder(d_model=16, strides=(2, 4), d_latent=64).to(dev).eval()      # widths 16 / 32: no 128-row LDS-DMA tile for the tail
    x = torch.randn(40, 1, 640, device=dev)
    z = enc(x)
    assert z.shape == (40, 64, 80) and torch.equal(z, enc.forward_plan(x))


SENTINEL = 0xA5                                                      # workspace bytes; outputs are pre-filled with OUT_SENTINEL
OUT_SENTINEL = -1234.5


def _refused(call, nbytes, room, outs):
    """`call(ws_ptr, ws_bytes)` with `nbytes` cut from a sentinel-filled buffer of `room` bytes must be refused with MVQ_EINVAL
    before anything is enqueued: no conv / residual-unit launch, the whole buffer and every output untouched."""
    from multimodal_vqvae_compression_audio_tactile_amd import _lib, ops
    L = _lib.lib()
    big = torch.full((room,), SENTINEL, dtype=torch.uint8, device=outs[0].device)
    before = [o.clone() for o in outs]
    ops.profile_begin()
    rc = call(big.data_ptr(), nbytes)
    launched = ops.profile_end()
    assert rc == -1 and b"workspace" in L.mvq_last_error(), (rc, L.mvq_last_error())
    assert launched == {}, launched
    assert bool((big == SENTINEL).all())
    for o, b in zip(outs, before):
        assert torch.equal(o, b)
    return big


@pytest.mark.parametrize("B", [1, 48])
def test_short_workspace_is_refused_before_any_launch(B, dev):
    """A workspace smaller than the plan needs is refused with MVQ_EINVAL and nothing launched, at the latency tiles (B = 1) and
    with the packed / virtually packed latent-rate rows (B = 48); the query's size runs and equals the module path.  The encoder's
    and the inference decoder's plans are the queries' largest, so one ALIGN (256 bytes) less is short; the decoder query also
    covers the saving forward and the backward, whose plans need about half of it, so those two get a quarter."""
    from multimodal_vqvae_compression_audio_tactile_amd import _lib, synth
    from multimodal_vqvae_compression_audio_tactile_amd.ops import _stream
    L = _lib.lib()
    mdl, _ = _models(dev)
    for p in mdl.decoder.parameters():
        p.requires_grad_(False)
    enc, dec = mdl.encoder.stack(), mdl.decoder.stack()
    x = synth.tactile_segments(B, seed=3).to(dev)
    T = x.shape[-1]
    z_ref = mdl.encoder(x)
    t = z_ref.shape[-1]
    q = L.mvq_encoder_workspace_bytes(enc.handle, B, T)
    z = torch.full_like(z_ref, OUT_SENTINEL)
    enc_call = lambda ws, n: L.mvq_encoder_fwd_f32(enc.handle, x.data_ptr(), z.data_ptr(), ws, n, B, T, _stream())
    big = _refused(enc_call, q - 256, q, [z])
    assert enc_call(big.data_ptr(), q) == 0 and torch.equal(z, z_ref)

    y_ref = mdl.decoder(z_ref)
    zz = z_ref.clone().requires_grad_(True)
    gy = torch.randn(y_ref.shape, generator=torch.Generator().manual_seed(B)).to(dev)
    mdl.decoder(zz).backward(gy)
    q = L.mvq_decoder_workspace_bytes(dec.handle, B, t)
    y = torch.full_like(y_ref, OUT_SENTINEL)
    dec_call = lambda ws, n: L.mvq_decoder_fwd_f32(dec.handle, z_ref.data_ptr(), y.data_ptr(), ws, n, B, t, _stream())
    big = _refused(dec_call, q - 256, q, [y])
    assert dec_call(big.data_ptr(), q) == 0 and torch.equal(y, y_ref)

    ns = L.mvq_decoder_saved_bytes(dec.handle, B, t)
    saved = torch.full((ns,), SENTINEL, dtype=torch.uint8, device=dev)
    y = torch.full_like(y_ref, OUT_SENTINEL)
    sav_call = lambda ws, n: L.mvq_decoder_fwd_saving_f32(dec.handle, z_ref.data_ptr(), y.data_ptr(), saved.data_ptr(), ns, ws, n, B, t, _stream())
    big = _refused(sav_call, q // 4, q, [y, saved])
    assert sav_call(big.data_ptr(), q) == 0 and torch.equal(y, y_ref)
    gz = torch.full_like(z_ref, OUT_SENTINEL)
    bwd_call = lambda ws, n: L.mvq_decoder_bwd_input_f32(dec.handle, saved.data_ptr(), ns, gy.data_ptr(), gz.data_ptr(), ws, n, B, t, _stream())
    big = _refused(bwd_call, q // 4, q, [gz, saved])
    assert bwd_call(big.data_ptr(), q) == 0 and torch.equal(gz, zz.grad)


def test_workspace_queried_before_set_plan_is_not_trusted(dev):
    """mvq_stack_set_plan(1, 1) switches the packed decoder head on at B = 1, t = 18 and so raises the workspace it needs
    (pinned in tests/test_abi_and_host.py).  A buffer sized before the switch is refused with nothing launched; ops.Stack forgets
    its cached size in set_plan, so the module path then runs and equals the Python plan under the same threshold."""
    from multimodal_vqvae_compression_audio_tactile_amd import _lib
    from multimodal_vqvae_compression_audio_tactile_amd.ops import _stream
    L = _lib.lib()
    mdl, _ = _models(dev)
    dec = mdl.decoder
    st = dec.stack()
    B, t = 1, 18
    z = torch.randn(B, 1024, t, generator=torch.Generator().manual_seed(18)).to(dev)
    st.decoder_fwd(z)                                                # caches the size of the default plan
    q_old = L.mvq_decoder_workspace_bytes(st.handle, B, t)
    assert st._ws_bytes[(B, t)] == q_old
    st.set_plan(vpack_min_batch=1, pack_min_batch=1)
    assert L.mvq_decoder_workspace_bytes(st.handle, B, t) > q_old
    y = torch.full((B, 1, st.out_len(t)), OUT_SENTINEL, device=dev)
    call = lambda ws, n: L.mvq_decoder_fwd_f32(st.handle, z.data_ptr(), y.data_ptr(), ws, n, B, t, _stream())
    _refused(call, q_old, q_old, [y])
    y = st.decoder_fwd(z)
    dec.PACK_MIN_BATCH = 1                                           # the Python plan under the same threshold
    assert dec._use_packed_latents(z)
    assert torch.equal(y, dec.forward_plan(z))
