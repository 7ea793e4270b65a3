"""No GPU: the host arithmetic of the rational streamed resampler and of the native-rate sender, and the argument checks of the two
exports mvq_resample_stream_rational_f32 / mvq_resample_stream_rational_slots_f32 (refused before any launch, null pointers)."""
import math
import random

import pytest

from multimodal_vqvae_compression_audio_tactile_amd import stream

# (orig_freq, new_freq) -> (orig, new, width): resample.sinc_resample_kernel's numbers, restated
RATIOS = {(3000, 24000): (1, 8, 7), (44100, 24000): (147, 80, 12), (24000, 44100): (80, 147, 7), (24000, 3000): (8, 1, 49)}
TOKEN_HOLD = {(3000, 24000): 40, (44100, 24000): 4, (24000, 44100): 4, (24000, 3000): 40}     # one 320-sample token at 24 kHz, in blocks


def test_the_restated_filter_numbers_are_the_designed_ones():
    from multimodal_vqvae_compression_audio_tactile_amd.resample import sinc_resample_kernel
    for (fi, fo), want in RATIOS.items():
        kern, width, orig, new = sinc_resample_kernel(fi, fo)
        assert (orig, new, width) == want and tuple(kern.shape) == (new, 2 * width + orig)
    assert RATIOS[(44100, 24000)][2] * 2 + 147 == 171 and RATIOS[(24000, 44100)][2] * 2 + 80 == 94 and 2 * 7 + 1 == 15


def _brute(consumed, n_new, orig, new, width, hold, final):
    """Outputs of the blocks this call completes: block q is complete once input q*orig + width + orig - 1 is in hand and q is at
    least ``hold`` blocks behind the newest whole input block, L/orig - 1; the final call writes every output up to ceil(new*L/orig)."""
    def blocks(L):
        return sum(1 for q in range(L // orig + 1) if q * orig + width + orig - 1 < L and q + hold <= L // orig - 1)
    before = blocks(consumed)
    if final:
        return math.ceil(new * (consumed + n_new) / orig) - new * before
    return new * (blocks(consumed + n_new) - before)


@pytest.mark.parametrize("ratio", sorted(RATIOS))
@pytest.mark.parametrize("token_hold", [False, True])
def test_out_len_equals_a_brute_force_count(ratio, token_hold):
    orig, new, width = RATIOS[ratio]
    hold = TOKEN_HOLD[ratio] if token_hold else None
    h = hold if hold is not None else -(-width // orig)
    assert h >= -(-width // orig)
    rng = random.Random(orig * 1000 + new + (7 if token_hold else 0))
    for trial in range(6):
        pieces = [orig * rng.randint(1, 3 * h + 5) for _ in range(rng.randint(0, 6))]
        ragged = rng.randint(0, 4 * orig + 3) if trial else 0                       # trial 0: an empty final piece (a flush)
        consumed, total = 0, 0
        for n in pieces:
            got = stream.resample_stream_rational_out_len(consumed, n, orig, new, width, hold)
            assert got == _brute(consumed, n, orig, new, width, h, False), (pieces, consumed, n)
            assert got % new == 0
            consumed, total = consumed + n, total + got
        got = stream.resample_stream_rational_out_len(consumed, ragged, orig, new, width, hold, final=True)
        assert got == _brute(consumed, ragged, orig, new, width, h, True), (pieces, ragged)
        assert total + got == math.ceil(new * (consumed + ragged) / orig)
        if new == 1 and not token_hold:
            c = 0
            for n in pieces:
                assert stream.resample_stream_rational_out_len(c, n, orig, new, width) == stream.resample_stream_out_len(c, n, orig, width)
                c += n
            assert stream.resample_stream_rational_out_len(c, ragged, orig, new, width, final=True) == \
                stream.resample_stream_out_len(c, ragged, orig, width, True)


def test_token_arithmetic_of_the_native_rate_sender():
    pa, pt = stream.native_token_plan(44100), stream.native_token_plan(3000)
    assert pa == (147, 80, 12, 4, 588, 600) and pt == (1, 8, 7, 40, 40, 47)         # orig, new, width, hold, samples per token, state
    for (orig, new, width, hold, tok, state) in (pa, pt):
        for m in range(1, 17):
            assert stream.resample_stream_rational_out_len(0, tok * m, orig, new, width, hold) == 320 * (m - 1)
            assert stream.resample_stream_rational_out_len(tok * 5, tok * m, orig, new, width, hold) == 320 * m
            assert stream.resample_stream_rational_out_len(tok, tok * m, orig, new, width, hold) == 320 * m
    with pytest.raises(ValueError, match="whole number"):
        stream.native_token_plan(2800)
    with pytest.raises(ValueError, match="1024"):
        stream.native_token_plan(96000)                                             # 4:1, hold 320 blocks of 4 samples: a state of 1305
    assert stream.native_token_plan(48000)[3:] == (320, 640, 653)


def test_sender_native_refuses_before_any_allocation():
    from multimodal_vqvae_compression_audio_tactile_amd import ProposedEval, StreamResampleRational, StreamSenderNative
    assert callable(ProposedEval.stream_sender_native) and StreamSenderNative is stream.StreamSenderNative and callable(StreamResampleRational)
    for rates, word in (((44100, 2800), "whole number"), ((2800, 3000), "whole number"), ((96000, 3000), "1024"), ((24000, 3000), "24000"),
                        ((44100,), "in_rates")):
        with pytest.raises(ValueError, match=word):
            StreamSenderNative(None, in_rates=rates)                                # the net is never looked at


RS_OK = dict(batch=1, n_new=588 * 2, consumed=0, final=0, len_out=320, orig=147, newf=80, width=12, ks=171, hold=4)


def _calls():
    """Both exports as f(**overrides of RS_OK) with null tensors (and a group of 1 in a pool of 4 for the slot form)."""
    from multimodal_vqvae_compression_audio_tactile_amd import _lib
    lib = _lib.lib()

    def dense(**kw):
        a = dict(RS_OK, **kw)
        return lib.mvq_resample_stream_rational_f32(None, None, None, None, a["batch"], a["n_new"], a["consumed"], a["final"], a["len_out"],
                                                    a["orig"], a["newf"], a["width"], a["ks"], a["hold"], None)

    def slots(n_slots=4, **kw):
        a = dict(RS_OK, **kw)
        return lib.mvq_resample_stream_rational_slots_f32(None, None, None, None, a["batch"], n_slots, None, a["n_new"], a["consumed"],
                                                          a["final"], a["len_out"], a["orig"], a["newf"], a["width"], a["ks"], a["hold"], None)
    return lib, dense, slots


def test_abi_argument_checks_of_both_exports():
    from multimodal_vqvae_compression_audio_tactile_amd import _lib
    lib, dense, slots = _calls()
    for n in ("mvq_resample_stream_rational_f32", "mvq_resample_stream_rational_slots_f32"):
        assert n in _lib.EXPORTS and hasattr(lib, n), n
    assert lib.mvq_abi_version() == 3
    for call in (dense, slots):
        assert call(ks=170) == -1 and b"2*width + orig" in lib.mvq_last_error()      # ks != 2*width + orig
        for neg in (dict(batch=-1), dict(n_new=-147), dict(consumed=-147), dict(len_out=-1), dict(width=-1, ks=145), dict(hold=-1),
                    dict(orig=0, ks=24), dict(newf=0)):
            assert call(**neg) == -1, neg                                           # negative sizes
        assert call(orig=1, newf=8, width=7, ks=15, hold=6, n_new=40, len_out=272) == -1 and b"ceil(width/orig)" in lib.mvq_last_error()
        assert call(consumed=100) == -1 and b"consumed" in lib.mvq_last_error()     # consumed % orig
        assert call(n_new=1177) == -1 and b"multiple" in lib.mvq_last_error()       # a non-final piece that is no multiple of orig
        assert call(len_out=321) == -1 and b"320" in lib.mvq_last_error()           # not the count the call completes
        assert call(len_out=400) == -1
        assert call(n_new=1177, final=1, len_out=640) == -1 and b"641" in lib.mvq_last_error()   # final: ceil(80*1177/147) = 641
        assert call() == -1 and b"null" in lib.mvq_last_error()                     # everything right but the tensors
        assert call(n_new=1177, final=1, len_out=641) == -1 and b"null" in lib.mvq_last_error()
        assert call(hold=7, len_out=0) == -2 and b"1024" in lib.mvq_last_error()    # S = 7*147 + 12 = 1041
        assert call(orig=1, newf=8, width=7, ks=15, hold=1018, n_new=40, len_out=0) == -2
        assert call(batch=0) == 0                                                   # empty: 0 without a launch
        assert call(batch=0, consumed=588 * 3, n_new=588, len_out=320) == 0         # steady: a token in, a token out
        assert call(batch=0, consumed=588 * 3, n_new=100, final=1, len_out=math.ceil(80 * 1864 / 147) - 80 * 8) == 0
    # the slot form's own refusals
    assert slots(batch=5) == -1 and b"pool of 4" in lib.mvq_last_error()            # a group larger than the pool
    assert slots(n_slots=-1) == -1 and slots(batch=-1) == -1
    assert slots(consumed=147, len_out=400) == -1 and b"launch class" in lib.mvq_last_error()   # inside the 600-sample state
    assert slots(consumed=588, n_new=588, len_out=320) == -1 and b"launch class" in lib.mvq_last_error()
    assert slots(batch=0, consumed=735, n_new=588, len_out=320) == 0                # 735 >= 600: the steady class
    assert dense(consumed=147, n_new=588, len_out=80) == -1 and b"null" in lib.mvq_last_error()  # the dense form takes any multiple of orig


def test_the_decimating_exports_still_refuse_other_ratios():
    from multimodal_vqvae_compression_audio_tactile_amd import _lib
    lib = _lib.lib()
    assert lib.mvq_resample_stream_f32(None, None, None, None, 1, 1920, 0, 0, 233, 8, 3, 49, 106, None) == -2
    assert b"decimation" in lib.mvq_last_error()
    assert lib.mvq_resample_stream_slots_f32(None, None, None, None, 1, 4, None, 1920, 0, 0, 233, 8, 3, 49, 106, None) == -2
    assert b"decimation" in lib.mvq_last_error()
