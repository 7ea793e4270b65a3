"""No GPU: the receiver's audio output --
  1. the yardstick agrees with itself: tests/audio_out_oracle.py's piece form (the receiver's schedule with the kernel's state row)
     concatenated equals its whole-item form, and both equal packets.AudioFade.apply, for every T, fade and mask the GPU tests use;
  2. the properties of the definition: untouched bits between gains of 1, +0 at gain 0 whatever the payload, g inside [0, 1];
  3. AudioFade's refusals; the new exports and their refusals before any launch;
  4. set_audio_decoder leaves the state dict alone, a strict load still succeeds with a decoder attached;
  5. the Python surface refuses audio_out without a decoder, audio_fade without audio_out and audio_out on the plain pool.
Every comparison is an equality."""
import inspect

import numpy as np
import pytest
import torch

import audio_out_oracle as ao
from multimodal_vqvae_compression_audio_tactile_amd import packets
from multimodal_vqvae_compression_audio_tactile_amd.packets import AudioFade

f32 = np.float32


def _bits(x):
    return np.ascontiguousarray(x, f32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ 1. the yardstick with itself
@pytest.mark.parametrize("H,F", ao.FADES)
@pytest.mark.parametrize("T", ao.TOKENS)
def test_pieces_equal_the_whole_item_and_the_definition(T, H, F):
    B = 3
    y = ao.payload(B, T, seed=T + 10 * H + F)
    for name, valid in ao.masks_for(B, T, H, F).items():
        want, gain = ao.whole(y, valid, H, F)
        got, states = ao.pieces(y, valid, H, F)
        assert got.shape == want.shape == (B, 320 * T - 8)
        assert np.array_equal(_bits(got), _bits(want)), (name, T, H, F)
        assert np.array_equal(_bits(AudioFade(H, F).apply(y[:, None], valid)[:, 0]), _bits(want)), name
        assert gain.min() >= 0 and gain.max() <= 1, name
        assert len(states) == T // 16 + 1
        for b in range(B):                                                       # the last state row: r of the item's last 11 tokens
            r = ao.runs(valid[b], H, F)
            tail = np.concatenate([np.zeros(ao.STATE, np.int64), r])[-ao.STATE:]
            assert np.array_equal(states[-1][b], tail), (name, b)
            assert np.array_equal(AudioFade(H, F).runs(valid[b]), r)
    # the masks are what their names say
    m = {k: ao.mask(k, T, H, F) for k in ao.MASKS}
    assert m["all"].all() and not m["none"].any() and m["first"][0] == 0 and m["last"][-1] == 0
    if T >= 37:
        lost = np.flatnonzero(m["long_run"] == 0)
        assert len(lost) == H + F + 3 > H + F and m["long_run"][lost[-1] + 1] != 0
        assert m["border_run"][15] == 0 and m["border_run"][16] == 0 and m["border_run"][12] != 0 and m["border_run"][20] != 0


def test_schedule_is_the_receivers():
    from multimodal_vqvae_compression_audio_tactile_amd import stream
    assert (ao.HOP, ao.TAIL, ao.HALO, ao.CHUNK) == (stream.HOP, stream.DEC_TAIL, stream.DEC_HALO_TOK, stream.CHUNK_TOK)
    for T in ao.TOKENS + [0, 15, 17, 32]:
        want = stream.schedule(T)
        got = [ao.piece_range(*s)[1:] for s in ao.steps(T)]
        assert got == [(e0, e1) for _, _, e0, e1 in want], T


# ------------------------------------------------------------------------------------------------ 2. properties of the definition
@pytest.mark.parametrize("H,F", ao.FADES)
def test_untouched_bits_and_predicated_zero(H, F):
    T, B = 37, 2
    valid = ao.masks_for(B, T, H, F)["long_run"]
    y = ao.payload(B, T, seed=5)
    _, gain = ao.whole(y, valid, H, F)
    one, zero = gain == 1, gain == 0
    assert one.any() and zero.any() and ((gain > 0) & (gain < 1)).any()
    yb = _bits(y).copy()
    for k, word in enumerate((0x7FC12345, 0x7149F2CA, 0x80000000)):              # a NaN with a payload, 1e30, -0
        yb[zero] = word
        yb.reshape(-1)[k::5][one.reshape(-1)[k::5]] = word
    y = yb.view(f32)
    assert np.isnan(y[zero]).any() or (y[zero] == 0).all()
    for got in (ao.whole(y, valid, H, F)[0], ao.pieces(y, valid, H, F)[0], AudioFade(H, F).apply(y, valid)):
        gb = _bits(got)
        assert np.array_equal(gb[one], yb[one])                                  # gain 1 on both sides: the sample keeps its bits
        assert not gb[zero].any()                                                # gain 0: +0, never NaN * 0 or -0
    # the fade shapes the names promise
    g = ao.gain_of(ao.runs(np.array([1, 0, 0, 0, 0, 0, 0, 1]), 1, 4), 1, 4)
    assert np.array_equal(g, np.array([1, 1, 0.75, 0.5, 0.25, 0, 0, 1], f32))    # repeat once, fade over four tokens
    g = ao.gain_of(ao.runs(np.array([1, 0, 0, 1]), 0, 1), 0, 1)
    assert np.array_equal(g, np.array([1, 0, 0, 1], f32))                        # mute with a one-token ramp


def test_audio_fade_refusals():
    for kw in (dict(hold_tok=-1), dict(fade_tok=0), dict(hold_tok=200, fade_tok=56), dict(hold_tok=1.0), dict(fade_tok=True)):
        with pytest.raises(ValueError, match="AudioFade"):
            AudioFade(**kw)
    assert AudioFade(0, 255) and AudioFade(254, 1) and AudioFade() == AudioFade(1, 4)
    with pytest.raises(ValueError, match="samples"):
        AudioFade().apply(np.zeros((1, 1, 320), f32), np.ones((1, 1), np.uint8))


# ------------------------------------------------------------------------------------------------ 3. exports and their refusals
def test_exports_refuse_before_any_launch():
    from multimodal_vqvae_compression_audio_tactile_amd import _lib, ops
    lib = _lib.lib()
    assert lib.mvq_abi_version() == 3
    one = 4096                                                                   # a non-null pointer; nothing is launched
    dense = lambda n, tok0, ln, H, F, y=one, v=one, st=one, B=1: lib.mvq_audio_fade_f32(y, v, st, B, n, tok0, ln, H, F, None)
    slots = lambda n, tok0, ln, H, F, G=1, S=4, sl=one: lib.mvq_audio_fade_slots_f32(one, one, one, sl, G, S, n, tok0, ln, H, F, None)
    for call in (dense, slots):
        assert call(16, 0, 1920, 1, 0) == -1 and b"fade_tok" in lib.mvq_last_error()
        assert call(16, 0, 1920, -1, 4) == -1
        assert call(16, 0, 1920, 200, 56) == -1
        assert call(16, 0, 1921, 1, 4) == -1 and b"len" in lib.mvq_last_error()
        assert call(16, 0, 1920 - 320, 1, 4) == -1                               # a push of 16 tokens emits at least 6
        assert call(16, 6, 1920, 1, 4) == -1                                     # a later piece reaches back 10 tokens
        assert call(16, 6, 320 * 17, 1, 4) == -1                                 # ... and no further
        assert call(-1, 0, 1920, 1, 4) == -1 and call(16, -1, 1920, 1, 4) == -1 and call(16, 0, -320, 1, 4) == -1
        assert call(11, 0, 320 * 10 - 8, 1, 4) == -1                             # a finish of 11 tokens makes at least 3512 samples
        assert call(11, 22, 320 * 22 - 8, 1, 4) == -1                            # ... and at most 21 tokens' worth
    assert dense(16, 0, 1920, 1, 4, y=None) == -1 and b"null" in lib.mvq_last_error()
    assert dense(16, 0, 1920, 1, 4, v=None) == -1 and dense(16, 0, 1920, 1, 4, st=None) == -1
    assert slots(16, 0, 1920, 1, 4, sl=None) == -1
    assert slots(16, 0, 1920, 1, 4, G=5, S=4) == -1                              # more sessions than slots
    assert dense(16, 0, 1920, 1, 4, y=None, v=None, st=None, B=0) == 0           # an empty batch launches nothing
    assert lib.mvq_audio_fade_slots_f32(None, None, None, None, 0, 4, 16, 0, 1920, 1, 4, None) == 0
    assert {"slots", "slots_dev"} <= set(inspect.signature(ops.audio_fade_).parameters)
    assert list(inspect.signature(ops.audio_fade_).parameters)[:5] == ["y", "valid", "state", "fade", "tok0"]
    st = ops.audio_fade_state(3, "cpu")
    assert st.shape == (3, ao.STATE) and st.dtype == torch.int32 and not st.any()
    import multimodal_vqvae_compression_audio_tactile_amd.torch_ops as T
    assert "audio_fade" in T.REGISTERED and hasattr(torch.ops.mi355x_vqvae, "audio_fade")
    m = lambda *s, dtype=torch.float32: torch.empty(*s, device="meta", dtype=dtype)
    assert torch.ops.mi355x_vqvae.audio_fade(m(2, 1, 1920), m(2, 16, dtype=torch.uint8), m(2, 11, dtype=torch.int32), 1, 4, 0) is None
    header = (_lib._PKG.parent / "include" / "mvq.h").read_text()
    assert "mvq_audio_fade_f32, mvq_audio_fade_slots_f32" in header.split("int mvq_abi_version")[0]


def test_ops_wrapper_refuses_on_the_host():
    from multimodal_vqvae_compression_audio_tactile_amd import MvqError, ops
    y, v, st = torch.zeros(2, 1, 1920), torch.ones(2, 16, dtype=torch.uint8), ops.audio_fade_state(2, "cpu")
    with pytest.raises(MvqError, match="AudioFade"):
        ops.audio_fade_(y, v, st, (1, 4), 0)
    with pytest.raises(MvqError, match="on the device"):
        ops.audio_fade_(y, v, st, AudioFade(), 0)


# ------------------------------------------------------------------------------------------------ 4. the decoder on the model
@pytest.fixture(scope="module")
def cpu_net():
    from multimodal_vqvae_compression_audio_tactile_amd import build_proposed
    return build_proposed(None, rvq_books=2, rvq_embed=128, device="cpu")


def test_set_audio_decoder_is_outside_the_state_dict(cpu_net):
    import golden_inputs as gi
    from multimodal_vqvae_compression_audio_tactile_amd import DAC, Decoder, build_proposed
    net = cpu_net
    keys = list(net.state_dict().keys())
    mods = [n for n, _ in net.named_modules()]
    assert net.audio_decoder is None
    dec = DAC().decoder
    assert net.set_audio_decoder(dec) is net and net.audio_decoder is dec
    assert list(net.state_dict().keys()) == keys and [n for n, _ in net.named_modules()] == mods
    assert not any(k.startswith(("A_DEC", "_audio")) for k in keys)
    assert not dec.training and not any(p.requires_grad for p in dec.parameters())
    net.load_state_dict(gi.model_state(7, 2, 128), strict=True)                  # a checkpoint holds no key of it
    assert net.audio_decoder is dec
    with pytest.raises(AttributeError):
        net.audio_decoder = dec                                                  # read-only: nothing gets registered
    assert list(net.state_dict().keys()) == keys
    for bad in (Decoder(rates=(8, 5, 4)), Decoder(channels=768), Decoder(output_padding=True)):
        with pytest.raises(ValueError, match="geometry"):
            net.set_audio_decoder(bad)
    for bad in (DAC(), torch.nn.Identity(), "decoder"):
        with pytest.raises(ValueError, match="dac.Decoder"):
            net.set_audio_decoder(bad)
    assert net.audio_decoder is dec                                              # a refusal leaves the attached one
    net.set_audio_decoder(None)
    assert net.audio_decoder is None
    assert inspect.signature(build_proposed).parameters["audio_decoder"].default is False
    with_dec = build_proposed(None, rvq_books=2, rvq_embed=128, device="cpu", audio_decoder=True)
    assert isinstance(with_dec.audio_decoder, Decoder) and with_dec.audio_decoder is not with_dec.T_DEC
    assert list(with_dec.state_dict().keys()) == keys


# ------------------------------------------------------------------------------------------------ 5. the surface's refusals
def test_surface_refusals(cpu_net):
    from multimodal_vqvae_compression_audio_tactile_amd import DAC, ProposedEval, ops, stream
    net = cpu_net
    net.set_audio_decoder(None)
    E = inspect.Parameter.empty
    for fn in (ProposedEval.decompress_packets_av, ProposedEval.stream_receiver, stream.StreamReceiver.__init__,
               stream.StreamReceiverPoolAV.__init__):
        p = inspect.signature(fn).parameters
        assert p["audio_out"].default is False and p["audio_fade"].default is None, fn
    assert inspect.signature(ProposedEval.decode_latents).parameters["return_qa"].default is False
    assert inspect.signature(ProposedEval.decode_av).parameters["audio_fade"].default is None
    assert inspect.signature(ProposedEval.decode_av).parameters["idx"].default is E
    info, ainfo = packets.StreamInfo(128, 2, 16, 2), packets.StreamInfo(1024, 32, 16, 2)
    makers = {"stream_receiver": lambda **kw: net.stream_receiver(128, 2, audio=(1024, 32), **kw),
              "StreamReceiverPoolAV": lambda **kw: stream.StreamReceiverPoolAV(net, 128, 2, audio=(1024, 32), slots=2, **kw),
              "decompress_packets_av": lambda **kw: net.decompress_packets_av([info], [[]], [ainfo], [[]], **kw)}
    for name, make in makers.items():
        with pytest.raises(ValueError, match="audio_out needs the audio decoder"):
            make(audio_out=True)
        with pytest.raises(ValueError, match="audio_fade .* goes with audio_out"):
            make(audio_fade=AudioFade())
    with pytest.raises(ValueError, match="audio_out needs the audio decoder"):
        net.decode_av(torch.zeros(1, 32, 16, dtype=torch.int64), torch.zeros(2, 1, 16, dtype=torch.int64))
    net.set_audio_decoder(DAC().decoder)
    try:
        for name, make in makers.items():
            with pytest.raises(ValueError, match="packets.AudioFade"):
                make(audio_out=True, audio_fade=(1, 4))
            with ops.arith("f16x3"):
                with pytest.raises(ValueError, match="arithmetic"):
                    make(audio_out=True)
        for kw in (dict(audio_out=True), dict(audio_fade=AudioFade())):          # the plain pool has no audio side at all
            with pytest.raises(ValueError, match="StreamReceiverPool: the pool has no audio output"):
                stream.StreamReceiverPool(net, 128, 2, **kw)
        # what audio_out allocates: a second decoder state and, with audio packets and a fade, the run lengths
        rx = net.stream_receiver(128, 2, batch=2, audio=(1024, 32), audio_out=True, audio_fade=AudioFade(0, 1))
        assert rx.a_hist.shape == rx.hist.shape == (2, 1024, 20) and rx.fade_state.shape == (2, 11) and rx.a_dec_state is None
        rx = net.stream_receiver(128, 2, audio_out=True, audio_fade=AudioFade())         # codes that arrive as codes lose nothing
        assert rx.a_hist is not None and rx.fade_state is None
        rx = net.stream_receiver(128, 2, audio=(1024, 32))
        assert rx.a_hist is None and rx.a_dec_state is None and rx.fade_state is None and not rx.audio_out
        pool = stream.StreamReceiverPoolAV(net, 128, 2, slots=3, audio=(1024, 32), audio_out=True, audio_fade=AudioFade())
        assert pool.a_hist.shape == (3, 1024, 20) and pool.fade_state.shape == (3, 11)
    finally:
        net.set_audio_decoder(None)
