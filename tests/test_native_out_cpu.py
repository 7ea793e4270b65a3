"""No GPU: the receiver's audio output at the playback rate --
  1. the split form's two exports exist and refuse, before any launch and with null pointers, with the one-block exports' codes;
  2. stream.native_out_plan: the admissible rates and the refusals, the rate named in the message;
  3. the five surfaces carry audio_out_rate=24000, the pinned factories do not, and all refuse with one message;
  4. the emitted pieces of stream.schedule(T) through resample_stream_rational_out_len sum to Resample's length: the condition the
     streaming equality rests on.
Every comparison is an equality."""
import inspect
import math

import pytest
import torch

from multimodal_vqvae_compression_audio_tactile_amd import packets, stream
from test_native_rate_cpu import RS_OK

# audio_out_rate -> (orig, new, width, hold, state): resample.sinc_resample_kernel(24000, rate)'s numbers at the smallest lag
PLANS = {44100: (80, 147, 7, 1, 87), 48000: (1, 2, 7, 7, 14), 22050: (160, 147, 7, 1, 167), 12000: (2, 1, 13, 7, 27),
         96000: (1, 4, 7, 7, 14)}
# the steady piece of the receiver at 44.1 kHz: 16 tokens in, 64 filter blocks of 147 outputs
OUT_OK = dict(batch=1, n_new=5120, consumed=7040, final=0, len_out=9408, orig=80, newf=147, width=7, ks=94, hold=1)


def _forms():
    """{form: (dense, slots)}: the exports as f(base, **overrides) with null tensors (a group of 1 in a pool of 4 for the slot form)."""
    from multimodal_vqvae_compression_audio_tactile_amd import _lib
    lib = _lib.lib()

    def make(dense_fn, slots_fn):
        def dense(base, **kw):
            a = dict(base, **kw)
            return dense_fn(None, None, None, None, a["batch"], a["n_new"], a["consumed"], a["final"], a["len_out"], a["orig"], a["newf"],
                            a["width"], a["ks"], a["hold"], None)

        def slots(base, n_slots=4, **kw):
            a = dict(base, **kw)
            return slots_fn(None, None, None, None, a["batch"], n_slots, None, a["n_new"], a["consumed"], a["final"], a["len_out"], a["orig"],
                            a["newf"], a["width"], a["ks"], a["hold"], None)
        return dense, slots
    return lib, {"block": make(lib.mvq_resample_stream_rational_f32, lib.mvq_resample_stream_rational_slots_f32),
                 "split": make(lib.mvq_resample_stream_rational_split_f32, lib.mvq_resample_stream_rational_split_slots_f32)}


# ------------------------------------------------------------------------------------------------------------ 1. exports
def test_split_exports_refuse_as_the_one_block_exports_do():
    from multimodal_vqvae_compression_audio_tactile_amd import _lib, ops, resample
    lib, forms = _forms()
    for n in ("mvq_resample_stream_rational_split_f32", "mvq_resample_stream_rational_split_slots_f32"):
        assert n in _lib.EXPORTS and hasattr(lib, n), n
    assert _lib.EXPORTS["mvq_resample_stream_rational_split_f32"] == _lib.EXPORTS["mvq_resample_stream_rational_f32"]
    assert _lib.EXPORTS["mvq_resample_stream_rational_split_slots_f32"] == _lib.EXPORTS["mvq_resample_stream_rational_slots_f32"]
    assert lib.mvq_abi_version() == 3
    cases = [(base, kw, word) for base in (RS_OK, OUT_OK) for kw, word in (
        (dict(ks=base["ks"] - 1), b"2*width + orig"),                               # ks != 2*width + orig
        (dict(hold=0), b"ceil(width/orig)"),                                        # hold too small
        (dict(consumed=base["consumed"] + 1), b"consumed"),                         # consumed % orig
        (dict(n_new=base["n_new"] + 1), b"multiple"),                               # a non-final piece that is no multiple of orig
        (dict(len_out=base["len_out"] + 1), b"len_out"),                            # not the count the call completes
        (dict(n_new=base["n_new"] + 1, final=1), b"len_out"),
        (dict(hold=13, len_out=0), b"1024"),                                        # S = 13*147 + 12 / 13*80 + 7 > 1024
        ({}, b"null"),                                                              # everything right but the tensors
        (dict(batch=0), None))]                                                     # empty: 0 without a launch
    for which in (0, 1):
        for base, kw, word in cases:
            want = forms["block"][which](base, **kw)
            want_msg = lib.mvq_last_error() if want else None
            got = forms["split"][which](base, **kw)
            assert got == want and want == (0 if word is None else -2 if word == b"1024" else -1), (which, kw, got, want)
            if word is not None:
                msg = lib.mvq_last_error()
                assert word in msg and word in want_msg, (kw, msg, want_msg)
                assert msg.replace(b"rational_split", b"rational") == want_msg          # the same message under the entry point's name
    # the slot form's own refusals
    for form in ("block", "split"):
        slots = forms[form][1]
        assert slots(OUT_OK, batch=5) == -1 and b"pool of 4" in lib.mvq_last_error()
        assert slots(OUT_OK, consumed=80, n_new=80, len_out=147) == -1 and b"launch class" in lib.mvq_last_error()   # inside the 87-sample state
        assert slots(OUT_OK, batch=0, consumed=1920) == 0
    # the Python faces: form= defaults to today's call, and a wrong one is refused on the host
    for fn in (ops.resample_stream_rational, ops.resample_stream_rational_slots, resample.StreamResampleRational.__init__):
        assert inspect.signature(fn).parameters["form"].default == "block", fn
    with pytest.raises(ops.MvqError, match="form"):
        resample.StreamResampleRational(24000, 44100, 1, device="cpu", form="parts")
    with pytest.raises(ops.MvqError, match="form"):
        ops.resample_stream_rational(torch.zeros(1, 80), torch.zeros(147, 94), torch.zeros(1, 87), 0, 80, 147, 7, form="parts")


# -------------------------------------------------------------------------------------------------------------- 2. rates
def test_admissible_rates():
    from multimodal_vqvae_compression_audio_tactile_amd.resample import sinc_resample_kernel
    assert stream.native_out_plan("x", 24000) is None and stream.native_out_plan("x", 24000, audio_out=False) is None
    for rate, want in PLANS.items():
        assert stream.native_out_plan("x", rate) == want, rate
        kern, width, orig, new = sinc_resample_kernel(24000, rate)
        assert (orig, new, width) == want[:3] and tuple(kern.shape) == (new, 2 * width + orig)
        assert want[3] == -(-width // orig) and want[4] == want[3] * orig + width <= 1024 and 320 % orig == 0
    assert 2 * 7 + 80 == 94 and 2 * 7 + 1 == 15 and 2 * 7 + 160 == 174                   # the banks' ks the issue names
    for rate in (16000, 32000, 8000):
        with pytest.raises(ValueError, match=f"^who: audio_out_rate = {rate} Hz .* whole number"):
            stream.native_out_plan("who", rate)
    with pytest.raises(ValueError, match="^who: audio_out_rate = 44100 Hz .* goes with audio_out=True"):
        stream.native_out_plan("who", 44100, audio_out=False)
    with pytest.raises(ValueError, match="^who: audio_out_rate = 44100 Hz .* 1024"):
        stream.native_out_plan("who", 44100, lowpass_filter_width=1000)                  # width 1011: a state of 1051 samples
    for bad in (0, -48000):
        with pytest.raises(ValueError, match="audio_out_rate"):
            stream.native_out_plan("who", bad)
    assert stream.audio_resample_form(1) in ("block", "split") and stream.audio_resample_form(1 << 20) in ("block", "split")


# ----------------------------------------------------------------------------------------------------------- 3. surfaces
@pytest.fixture(scope="module")
def cpu_net():
    from multimodal_vqvae_compression_audio_tactile_amd import build_proposed
    return build_proposed(None, rvq_books=2, rvq_embed=128, device="cpu")


def test_five_surfaces(cpu_net):
    from multimodal_vqvae_compression_audio_tactile_amd import DAC, ProposedEval
    from multimodal_vqvae_compression_audio_tactile_amd.packets import AudioFade
    net = cpu_net
    for fn in (ProposedEval.stream_receiver, stream.StreamReceiver.__init__, stream.StreamReceiverPoolAV.__init__,
               ProposedEval.decompress_packets_av, ProposedEval.decode_av):
        assert inspect.signature(fn).parameters["audio_out_rate"].default == 24000, fn
    for fn in (ProposedEval.stream_receiver_pool_av, ProposedEval.stream_receiver_pool, stream.StreamReceiverPool.__init__):
        assert "audio_out_rate" not in inspect.signature(fn).parameters, fn             # the pinned factories stay as they are
    info, ainfo = packets.StreamInfo(128, 2, 16, 2), packets.StreamInfo(1024, 32, 16, 2)
    codes, idx = torch.zeros(1, 32, 16, dtype=torch.int64), torch.zeros(2, 1, 16, dtype=torch.int64)
    makers = {"stream_receiver": lambda **kw: net.stream_receiver(128, 2, audio=(1024, 32), **kw),
              "StreamReceiver": lambda **kw: stream.StreamReceiver(net, 128, 2, audio=(1024, 32), **kw),
              "StreamReceiverPoolAV": lambda **kw: stream.StreamReceiverPoolAV(net, 128, 2, audio=(1024, 32), slots=2, **kw),
              "decompress_packets_av": lambda **kw: net.decompress_packets_av([info], [[]], [ainfo], [[]], **kw)}
    name_in_front = {"stream_receiver": "StreamReceiver"}
    net.set_audio_decoder(DAC().decoder)
    try:
        said = {16000: set(), 32000: set(), 8000: set()}                                # per rate: the messages without the caller's name
        for name, make in makers.items():
            who = name_in_front.get(name, name)
            with pytest.raises(ValueError, match=f"^{who}: audio_out_rate = 44100 Hz .* goes with audio_out=True"):
                make(audio_out_rate=44100)
            for rate in (16000, 32000, 8000):
                with pytest.raises(ValueError, match=f"^{who}: audio_out_rate = {rate} Hz") as e:
                    make(audio_out=True, audio_out_rate=rate)
                said[rate].add(str(e.value)[len(who):])
        with pytest.raises(ValueError, match="^decode_av: audio_out_rate = 16000 Hz") as e:      # decode_av is audio_out by definition
            net.decode_av(codes, idx, audio_out_rate=16000)
        said[16000].add(str(e.value)[len("decode_av"):])
        assert all(len(v) == 1 and "whole number" in next(iter(v)) for v in said.values()), said   # one message on all five
        # what the rate allocates, before any device call: the second resampler state at the smallest lag
        rx = net.stream_receiver(128, 2, batch=2, audio=(1024, 32), audio_out=True, audio_fade=AudioFade(), audio_out_rate=44100)
        assert rx.ars_state.shape == (2, 87) and not rx.ars_state.any() and rx.ars_kernel.shape == (147, 94) and rx.rs_state is None
        rx = net.stream_receiver(128, 2, audio=(1024, 32), audio_out=True, out_rate=3000, audio_out_rate=48000)
        assert rx.ars_state.shape == (1, 14) and rx.rs_state.shape == (1, 105)
        rx = net.stream_receiver(128, 2, audio=(1024, 32), audio_out=True)
        assert rx.ars_state is None and rx.ars_kernel is None and rx.audio_out_rate == 24000
        pool = stream.StreamReceiverPoolAV(net, 128, 2, slots=3, audio=(1024, 32), audio_out=True, audio_out_rate=22050)
        assert pool.ars_state.shape == (3, 167)
        pool.ars_state.fill_(float("nan"))
        sid = pool.open()
        assert not pool.ars_state[0].any() and bool(torch.isnan(pool.ars_state[1:]).all())   # open() zeroes the slot's row only
        pool.close(sid)
        with pytest.raises(ValueError, match="out_rate must be"):                       # out_rate keeps its two values
            net.stream_receiver(128, 2, audio=(1024, 32), audio_out=True, out_rate=8000, audio_out_rate=44100)
    finally:
        net.set_audio_decoder(None)


# ------------------------------------------------------------------------------------------------------------- 4. pieces
@pytest.mark.parametrize("rate", [44100, 48000, 22050])
def test_emitted_pieces_sum_to_the_whole_item_length(rate):
    orig, new, width, hold, state = PLANS[rate]
    for T in (1, 6, 11, 16, 17, 37, 75):
        steps = stream.schedule(T)
        consumed, total = 0, 0
        for k, (_, _, e0, e1) in enumerate(steps):
            last = k == len(steps) - 1
            assert e0 == consumed and (last or ((e1 - e0) % 320 == 0 and e1 > e0))      # whole tokens, so whole filter blocks
            assert consumed == 0 or consumed >= 1920 > state                            # a launch class of a pool group
            n_out = stream.resample_stream_rational_out_len(consumed, e1 - e0, orig, new, width, hold, final=last)
            assert last or n_out % new == 0
            consumed, total = e1, total + n_out
        assert consumed == 320 * T - 8
        assert total == math.ceil(new * (320 * T - 8) / orig) == -(-new * (320 * T - 8) // orig), (rate, T)
