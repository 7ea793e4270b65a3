"""CPU: the streaming receiver's host logic and the arithmetic facts it rests on, restated from oracle pieces
(tests/stream_oracle.py).

  * the window schedule tiles the output exactly once, in order, and keeps every emitted sample a halo away from a window edge;
  * T_DEC over that schedule equals the one-shot decode bit for bit on the oracle (and no longer does with a halo of 9 tokens);
  * the receiver loop run one chunk per call with the last token carried equals the whole-item loop under every loss pattern;
  * output n of the resampler needs input sample 8n + 56 and nothing later;
  * gather(seq_base=), the constructor's refusals, the late-packet count, the new entry points' argument checks."""
import numpy as np
import pytest
import torch

import lossy_oracle as lo
import stream_oracle as so
from multimodal_vqvae_compression_audio_tactile_amd import packets, stream, synth
from multimodal_vqvae_compression_audio_tactile_amd.packets import StreamInfo

_ONE_SHOT = {}


# ---------------------------------------------------------------------------------------------------------- 1. schedule
def test_schedule_tiles_the_output_and_keeps_the_halo():
    assert (stream.DEC_HALO_TOK, stream.DEC_HALO_SAMPLES, stream.ENC_HALO_TOK) == (10, (3132, 3141), 8)
    assert stream.HOP * stream.DEC_HALO_TOK >= max(stream.DEC_HALO_SAMPLES)
    for T in range(1, 101):
        steps = stream.schedule(T)
        assert len(steps) == T // 16 + 1                             # one per full chunk, then finish
        pos = 0
        for a, b, e0, e1 in steps:
            assert 0 <= a <= b <= T and e0 == pos and e1 >= e0        # in order, no gap, no overlap
            pos = e1
            if e1 > e0:
                assert _margins_ok(a, b, e0, e1, T)
        assert pos == 320 * T - 8
        assert [b for _, b, _, _ in steps[:-1]] == list(range(16, T + 1, 16)) and steps[-1][1] == T
    lens = [b - a for a, b, _, _ in stream.schedule(96)]
    assert lens == [16, 32, 36, 36, 36, 36, 20]
    assert stream.schedule(0) == [(0, 0, 0, 0)]
    with pytest.raises(ValueError):
        stream.schedule(-1)


def _margins_ok(a, b, e0, e1, T):
    """Every emitted sample is >= 3132 samples from a window start that is not token 0 and >= 3141 from a window end that is not
    T (the window's output has 320*(b-a) - 8 samples)."""
    lo_ok = a == 0 or e0 - 320 * a >= stream.DEC_HALO_SAMPLES[0]
    hi_ok = b == T or (320 * b - 8) - e1 >= stream.DEC_HALO_SAMPLES[1]
    return lo_ok and hi_ok and e0 >= 320 * a and e1 <= 320 * b - 8


# ------------------------------------------------------------------------------------------- 2. window decode on the oracle
def _one_shot(orc, T):
    if T not in _ONE_SHOT:
        sd = so.dec_weights(7)
        z = so.latents(T)
        _ONE_SHOT[T] = (sd, z, orc.dac_decoder(sd, z, prefix="decoder."))
    return _ONE_SHOT[T]


@pytest.mark.parametrize("T", [11, 16, 37, 75])
def test_oracle_window_decode_equals_one_shot(T, orc):
    sd, z, whole = _one_shot(orc, T)
    assert z.shape == (2, 1024, T) and whole.shape == (2, 1, 320 * T - 8)
    got = so.windowed_decode(orc, sd, z, stream.schedule(T))
    assert got.shape == whole.shape and np.array_equal(got, whole)


def test_oracle_window_decode_needs_the_ten_token_halo(orc):
    sd, z, whole = _one_shot(orc, 75)
    got = so.windowed_decode(orc, sd, z, stream.schedule(75, halo=9))
    assert got.shape == whole.shape and not np.array_equal(got, whole)


# ---------------------------------------------------------------------------------------------------- 3. carried token
@pytest.fixture(scope="module")
def head_sd():
    return {k: v.numpy() for k, v in synth.proposed_head_state(17, rvq_books=3, rvq_embed=128).items()}


@pytest.mark.parametrize("B,Tlat", [(2, 37), (1, 75), (1, 16), (1, 11)])
def test_chunk_at_a_time_with_the_carried_token_equals_the_whole_item(B, Tlat, orc, head_sd):
    r = np.random.default_rng(Tlat * 10 + B)
    qa = (0.5 * r.standard_normal((B, 1024, Tlat))).astype(np.float32)
    idx = r.integers(0, 128, size=(3, B, Tlat))
    for name in lo.PATTERNS:
        nbv = lo.loss_pattern(name, B, Tlat, 3)
        want = lo.lossy_loop(orc, head_sd, qa, idx, nbv)
        assert np.array_equal(so.chunked_latents(orc, head_sd, qa, idx, nbv), want), name


# ------------------------------------------------------------------------------------------------ 4. resampler contract
def test_resampler_output_n_needs_sample_8n_plus_56(orc):
    from multimodal_vqvae_compression_audio_tactile_amd import ops
    from multimodal_vqvae_compression_audio_tactile_amd.resample import sinc_resample_kernel
    _, width, orig, new = sinc_resample_kernel(24000, 3000)
    assert (width, orig, new) == (49, 8, 1) and 2 * width + orig == 106
    L = 13752
    x = np.random.default_rng(3).standard_normal((2, L)).astype(np.float32)
    whole = orc.resample(x, 24000, 3000)
    assert whole.shape == (2, 1719)
    for n in (1920, 7040, 13752):
        part = orc.resample(x[:, :n], 24000, 3000)
        ready = max(0, (n - 57) // 8 + 1) if n >= 57 else 0           # outputs with 8n + 56 < len(prefix)
        assert np.array_equal(part[:, :ready], whole[:, :ready])
        if n < L:
            assert not np.array_equal(part[:, :ready + 7], whole[:, :ready + 7])      # ... and the next ones are not final yet
            # the count the streamed kernel emits is exactly the ready ones
            assert sum(ops.resample_stream_out_len(c, m, 8, 49) for c, m in _pieces(n)) == ready
    assert ops.resample_stream_out_len(12160, 1592, 8, 49, final=True) + (12160 // 8 - 7) == 1719
    assert ops.resample_stream_out_len(0, 3512, 8, 49, final=True) == 439
    assert ops.resample_stream_state(8, 49, 3, "cpu").shape == (3, 105)


def _pieces(n):
    """n samples in the streaming receiver's emit lengths."""
    out, c = [], 0
    for m in [1920] + [5120] * 10:
        if c + m > n:
            break
        out.append((c, m))
        c += m
    assert c == n
    return out


# ----------------------------------------------------------------------------------------------------- 5. host logic
def test_gather_seq_base_rebases_and_validates():
    whole = StreamInfo(512, 8, 37, 2)
    idx = np.random.default_rng(1).integers(0, 512, size=(8, 37))
    pk = packets.frame(packets.pack_bodies(idx, whole), whole)
    assert len(pk) == 19
    # chunk 1 (tokens 16..31) carries the stream's packets 8..15; the tail chunk (5 tokens) 16..18, the last with one token
    c1 = StreamInfo(512, 8, 16, 2)
    bodies, recv = packets.gather(pk[8:16][::-1], c1, seq_base=8)
    back, nbv = packets.unpack_bodies(bodies, recv, c1)
    assert np.array_equal(back, idx[:, 16:32]) and np.all(nbv == 8)
    tail = StreamInfo(512, 8, 5, 2)
    bodies, recv = packets.gather(pk[16:], tail, seq_base=16)
    back, _ = packets.unpack_bodies(bodies, recv, tail)
    assert np.array_equal(back, idx[:, 32:])
    # missing and thinned packets of the chunk
    bodies, recv = packets.gather([pk[9], packets.thin(pk[12], 3, whole)], c1, seq_base=8)
    assert recv.tolist() == [0, 8, 0, 0, 3, 0, 0, 0]
    # a packet of an earlier chunk: refused, or collected when the caller asks for that
    with pytest.raises(ValueError, match="seq_base"):
        packets.gather([pk[9], pk[7]], c1, seq_base=8)
    late = []
    bodies, recv = packets.gather([pk[9], pk[7], pk[0]], c1, seq_base=8, late=late)
    assert late == [pk[7], pk[0]] and recv.tolist() == [0, 8, 0, 0, 0, 0, 0, 0]
    # a packet of a later chunk, and the tail packet's token count inside a full chunk
    with pytest.raises(ValueError, match="seq 16"):
        packets.gather([pk[16]], c1, seq_base=8, late=[])
    with pytest.raises(ValueError, match="ntok"):
        packets.gather([pk[18]], StreamInfo(512, 8, 6, 2), seq_base=16)
    with pytest.raises(ValueError):
        packets.gather([], c1, seq_base=-1)
    with pytest.raises(ValueError):
        packets.gather([], c1, seq_base=2 ** 32 - 7)
    # the default is today's call
    a, b = packets.gather(pk, whole)
    c, d = packets.gather(pk, whole, seq_base=0)
    assert np.array_equal(a, c) and np.array_equal(b, d)


@pytest.fixture(scope="module")
def cpu_net():
    from multimodal_vqvae_compression_audio_tactile_amd import build_proposed
    return build_proposed(None, rvq_books=2, rvq_embed=128, device="cpu")


def test_stream_receiver_refusals_come_before_any_launch(cpu_net):
    """On a CPU-resident model nothing can have been launched: the checks come first."""
    from multimodal_vqvae_compression_audio_tactile_amd import MvqError
    net = cpu_net
    for ptok in (3, 5, 32, 0):
        with pytest.raises(ValueError, match="does not divide"):
            net.stream_receiver(128, 2, packet_tok=ptok)
    with pytest.raises(ValueError, match="plc"):
        net.stream_receiver(128, 2, conceal="plc")
    with pytest.raises(ValueError, match="conceal"):
        net.stream_receiver(128, 2, conceal="interpolate")
    with pytest.raises(ValueError, match="K = 512"):
        net.stream_receiver(512, 2)
    with pytest.raises(ValueError, match="out_rate"):
        net.stream_receiver(128, 2, out_rate=8000)
    with pytest.raises(ValueError, match="batch"):
        net.stream_receiver(128, 2, batch=0)
    rx = net.stream_receiver(128, 2, batch=2)
    assert isinstance(rx, stream.StreamReceiver) and (rx.tokens, rx.late, rx.finished) == (0, 0, False)
    codes = torch.zeros(2, 32, 16, dtype=torch.int64)
    with pytest.raises(ValueError, match="batch"):
        rx.push([[]], codes)
    with pytest.raises(ValueError, match="audio"):
        rx.push([[], []], codes[:1])
    with pytest.raises(ValueError, match="15 audio tokens"):
        rx.push([[], []], codes[..., :15])
    with pytest.raises(ValueError, match="audio"):
        rx.push([[], []], codes.float())
    with pytest.raises(ValueError, match="16 audio tokens"):
        rx.finish([[], []], codes)
    with pytest.raises(ValueError, match="both"):
        rx.finish([[], []])
    info = StreamInfo(128, 2, 32, 2)
    pk = packets.frame(packets.pack_bodies(np.zeros((2, 32), np.int64), info), info)
    with pytest.raises(ValueError, match="seq 8"):                   # a packet of the next chunk
        rx.push([[pk[0]], [pk[8]]], codes)
    assert rx.tokens == 0
    rx.finished = True
    with pytest.raises(MvqError, match="after finish"):
        rx.push([[], []], codes)
    with pytest.raises(MvqError, match="after finish"):
        rx.finish()
    # the carried token: not with the whole-sequence concealment, not without a recursion, and of the right shape
    idx = torch.zeros(2, 2, 16, dtype=torch.int64)
    z = torch.zeros(2, 1024)
    full = torch.full((2, 16), 2, dtype=torch.uint8)
    with pytest.raises(MvqError, match="z_prev"):
        net.decode_latents(codes, idx, nb_valid=full, conceal="plc", plc=net, z_prev=z)
    with pytest.raises(MvqError, match="tactile_only"):
        net.decode_latents(None, idx, tactile_only=True, z_prev=z)
    with pytest.raises(MvqError, match="tactile_only"):
        net.decode_latents(None, idx, tactile_only=True, z_last_out=z)
    for bad in (z[:1], z.double(), torch.zeros(2, 1024, 1), torch.zeros(1024, 2).t()):
        with pytest.raises(MvqError, match="z_prev must be"):
            net.decode_latents(codes, idx, z_prev=bad)


def test_late_packets_are_counted_and_ignored(cpu_net):
    rx = cpu_net.stream_receiver(128, 2, batch=2)
    info = StreamInfo(128, 2, 48, 2)
    idx = np.random.default_rng(2).integers(0, 128, size=(2, 48))
    pk = packets.frame(packets.pack_bodies(idx, info), info)
    rx.tokens, rx.h = 32, 20                                         # two chunks decoded: chunk 2 carries packets 16..23
    host = rx._gather([pk[16:24] + [pk[3], pk[15]], [pk[0], pk[20]]], 16)
    assert rx.late == 3
    full = packets.body_bytes(2, 2, 128)
    bodies, recv = host[:2 * 8 * full].reshape(2, 8, full), host[2 * 8 * full:].reshape(2, 8)
    assert recv.tolist() == [[2] * 8, [0, 0, 0, 0, 2, 0, 0, 0]]
    back, _ = packets.unpack_bodies(bodies[0], recv[0], StreamInfo(128, 2, 16, 2))
    assert np.array_equal(back, idx[:, 32:48])
    assert rx._plan(16, False) == (20, 20, 3200, 8320) and rx._plan(5, True) == (20, 20, 3200, 7992)


def test_stream_entry_points_check_their_arguments():
    from multimodal_vqvae_compression_audio_tactile_amd import ProposedEval, StreamReceiver, StreamResample, _lib, ops
    assert callable(ProposedEval.stream_receiver) and StreamReceiver is stream.StreamReceiver and callable(StreamResample)
    for n in ("stream_window", "resample_stream"):
        assert callable(getattr(ops, n, None)), n
    lib = _lib.lib()
    for n in ("mvq_stream_window_f32", "mvq_resample_stream_f32"):
        assert n in _lib.EXPORTS and hasattr(lib, n), n
    assert lib.mvq_abi_version() == 3
    # refused before any device access (no GPU here)
    win = lib.mvq_stream_window_f32
    assert win(None, 16, None, 16, None, 33, 40, 1, 96, None) == -1            # h_out > h_in + n
    assert b"exceeds h_in + n" in lib.mvq_last_error()
    assert win(None, 21, None, 16, None, 20, 20, 1, 96, None) == -1            # past the capacity
    assert win(None, 16, None, 16, None, 21, 20, 1, 96, None) == -1
    for neg in ((-1, 16, 16, 20, 1, 96), (16, -1, 16, 20, 1, 96), (16, 16, -1, 20, 1, 96), (16, 16, 16, -1, 1, 96), (16, 16, 16, 20, -1, 96),
                (16, 16, 16, 20, 1, -96)):
        assert win(None, neg[0], None, neg[1], None, neg[2], neg[3], neg[4], neg[5], None) == -1
    assert win(None, 16, None, 16, None, 20, 20, 1, 96, None) == -1            # null pointers, non-empty shape
    assert b"null" in lib.mvq_last_error()
    assert win(None, 16, None, 16, None, 20, 20, 0, 96, None) == 0             # empty: 0 without a launch
    assert win(None, 0, None, 0, None, 0, 20, 1, 96, None) == 0
    rs = lib.mvq_resample_stream_f32
    assert rs(None, None, None, None, 1, 1920, 0, 0, 233, 8, 3, 49, 106, None) == -2          # not a pure decimation
    assert rs(None, None, None, None, 1, 1921, 0, 0, 233, 8, 1, 49, 106, None) == -1          # a piece that is no multiple of 8
    assert b"multiple" in lib.mvq_last_error()
    assert rs(None, None, None, None, 1, 1920, 4, 0, 233, 8, 1, 49, 106, None) == -1          # nor the samples before it
    assert rs(None, None, None, None, 1, 1920, 0, 0, 233, 8, 1, 49, 105, None) == -1          # ks != 2*width + orig
    assert rs(None, None, None, None, 1, 1920, 0, 0, 240, 8, 1, 49, 106, None) == -1          # 233 outputs are complete, not 240
    assert b"233" in lib.mvq_last_error()
    assert rs(None, None, None, None, 1, 1920, 0, 0, 233, 8, 1, 49, 106, None) == -1          # null tensors
    assert rs(None, None, None, None, 0, 1920, 0, 0, 233, 8, 1, 49, 106, None) == 0           # empty batch
    assert rs(None, None, None, None, 0, 1921, 1920, 1, 248, 8, 1, 49, 106, None) == 0        # final: ceil(3841/8) - 233
    assert rs(None, None, None, None, 0, 8, 0, 0, 0, 8, 1, 520, 1048, None) == -2             # a state beyond 1024 samples
