"""CPU: the streaming sender's host logic and the arithmetic facts it rests on, restated from oracle pieces
(tests/sender_oracle.py).

  * the push schedule emits every chunk once and in order, at most one per push, every emitted token 8 tokens inside a window
    edge that is not the item's, never more than 47 tokens of samples held, 32-token windows in the steady state;
  * the encoder over that schedule equals the whole-item encode bit for bit on the oracle (and no longer does with a halo of 7);
  * the quantisation loop run one chunk per call with the last token carried equals the whole-item loop (indices and z_run);
  * frame(seq_base=): per-chunk packets concatenated are the whole item's; the session's and the new entry points' refusals."""
import numpy as np
import pytest
import torch

import sender_oracle as sn
from multimodal_vqvae_compression_audio_tactile_amd import packets, stream, synth
from multimodal_vqvae_compression_audio_tactile_amd.packets import StreamInfo

_WHOLE = {}


# ---------------------------------------------------------------------------------------------------------- 1. schedule
def _patterns(T):
    r = np.random.default_rng(T)
    mixed, used = [], 0
    while True:
        m = int(r.integers(1, 17))
        if used + m > T:
            break
        mixed.append(m)
        used += m
    return {"all16": [16] * (T // 16), "all1": [1] * T, "mixed": mixed}


def test_sender_schedule_tiles_the_item_and_keeps_the_halo():
    assert (stream.ENC_HALO_TOK, stream.PUSH_MAX_TOK, stream.SEND_CAP_TOK, stream.CHUNK_TOK) == (8, 16, 48, 16)
    for T in range(1, 101):
        for name, pushes in _patterns(T).items():
            steps = stream.sender_schedule(T, pushes)
            assert len(steps) == len(pushes) + 1, (T, name)
            nxt, have, start = 0, 0, 0
            for i, (w0, w1, c0, c1, held) in enumerate(steps):
                fin = i == len(pushes)
                have = T if fin else have + pushes[i]
                assert c0 == nxt and c1 >= c0, (T, name, i)                          # in order, no gap, no overlap
                assert fin or c1 - c0 <= 1                                            # a push emits at most one chunk
                assert have - start <= 47 or fin                                      # samples held before the step drops any
                if c1 > c0:
                    e0, e1 = 16 * c0, min(16 * c1, T)
                    assert w0 == start and w0 <= e0 and e1 <= w1 <= have
                    assert w0 == 0 or e0 - w0 >= 8                                    # 8 tokens inside the window's start ...
                    assert (fin and w1 == T) or w1 - e1 >= 8                          # ... and its end, unless that is the item's
                    if not fin:
                        assert w1 - w0 == (24 if c0 == 0 else 32)                     # the steady window: twice the tokens emitted
                        start = 16 * c1 - 8
                else:
                    assert w0 == w1
                assert held == (0 if fin else have - start) and held <= 47
                nxt = c1
            assert nxt == -(-T // 16), (T, name)                                      # every chunk, the partial one too
            assert steps[-1][3] - steps[-1][2] <= 3                                   # finish flushes at most three chunks
    assert [s[:4] for s in stream.sender_schedule(96, [16] * 6)] == \
        [(0, 0, 0, 0), (0, 24, 0, 1), (8, 40, 1, 2), (24, 56, 2, 3), (40, 72, 3, 4), (56, 88, 4, 5), (72, 96, 5, 6)]
    assert stream.sender_schedule(0, []) == [(0, 0, 0, 0, 0)]
    for bad in ((-1, []), (10, [17]), (10, [0]), (10, [8, 8])):
        with pytest.raises(ValueError):
            stream.sender_schedule(*bad)
    assert [stream.enc_tokens(n) for n in (0, 100, 320, 5120, 24000, 320 * 40 - 137)] == [0, 0, 1, 16, 75, 39]


# ------------------------------------------------------------------------------------------ 2. window encode on the oracle
def _whole(orc, L):
    if L not in _WHOLE:
        sd = sn.enc_weights(7)
        x = sn.signal(L)
        _WHOLE[L] = (sd, x, orc.dac_encoder(sd, x, prefix="encoder."))
    return _WHOLE[L]


@pytest.mark.parametrize("L", [320 * 11, 320 * 16, 320 * 37, 24000, 320 * 40 - 137])
def test_oracle_window_encode_equals_whole_item(L, orc):
    sd, x, whole = _whole(orc, L)
    assert whole.shape == (1, 1024, stream.enc_tokens(L))
    got = sn.scheduled_encode(orc, sd, x, sn.split_pushes(L, 16))
    assert got.shape == whole.shape and np.array_equal(got, whole)


def test_oracle_window_encode_needs_the_eight_token_halo(orc):
    sd, x, whole = _whole(orc, 24000)
    got = sn.scheduled_encode(orc, sd, x, sn.split_pushes(24000, 16), halo=7)
    assert got.shape == whole.shape and not np.array_equal(got, whole)
    diff = np.flatnonzero(np.any(got != whole, axis=(0, 1)))
    assert set(diff.tolist()) <= {15, 16, 31, 32, 47, 48, 63, 64} and diff.size


# ---------------------------------------------------------------------------------------------------- 3. carried token
@pytest.fixture(scope="module")
def model_sd():
    return {k: v.numpy() for k, v in synth.proposed_model_state(17, rvq_books=3, rvq_embed=128).items()}


@pytest.mark.parametrize("B,Tlat", [(2, 37), (1, 75), (1, 16), (1, 11)])
def test_ar_chunk_at_a_time_with_the_carried_token_equals_the_whole_item(B, Tlat, orc, model_sd):
    a = synth.audio_segments(B, seed=Tlat, T=320 * Tlat).numpy()
    t = synth.tactile_segments(B, seed=Tlat, T=320 * Tlat).numpy()
    z_run, aux = orc.proposed_encode_latents(model_sd, a, t, return_aux=True)
    assert z_run.shape == (B, 1024, Tlat) and aux["idx"].shape == (3, B, Tlat)
    got_z, got_idx = sn.chunked_ar(orc, model_sd, aux["qa"], aux["zt"])
    assert np.array_equal(got_idx, aux["idx"]) and np.array_equal(got_z, z_run)


# ----------------------------------------------------------------------------------------------------------- 4. framing
def test_frame_seq_base_numbers_a_chunk_as_the_stream_does():
    for T, ptok in ((37, 2), (75, 4), (16, 16), (11, 1)):
        whole = StreamInfo(512, 8, T, ptok)
        idx = np.random.default_rng(T).integers(0, 512, size=(8, T))
        want = packets.frame(packets.pack_bodies(idx, whole), whole)
        assert packets.frame(packets.pack_bodies(idx, whole), whole, seq_base=0) == want         # the default is today's output
        got = []
        for s in range(0, T, 16):
            e = min(T, s + 16)
            info = StreamInfo(512, 8, e - s, ptok)
            got += packets.frame(packets.pack_bodies(idx[:, s:e], info), info, seq_base=s // ptok)
        assert got == want
        # ... and gather(seq_base=) takes them back
        info = StreamInfo(512, 8, min(16, T), ptok)
        bodies, recv = packets.gather(packets.frame(packets.pack_bodies(idx[:, :info.T], info), info, seq_base=40), info, seq_base=40)
        assert np.array_equal(packets.unpack_bodies(bodies, recv, info)[0], idx[:, :info.T])
    info = StreamInfo(512, 8, 16, 2)
    z = np.zeros((8, 16), np.int64)
    for bad in (-1, 2 ** 32 - 7):
        with pytest.raises(ValueError, match="seq_base"):
            packets.frame(packets.pack_bodies(z, info), info, seq_base=bad)
    assert packets.frame(packets.pack_bodies(z, info), info, seq_base=2 ** 32 - 8)[-1][3:7] == b"\xff\xff\xff\xff"


# ---------------------------------------------------------------------------------------------------------- 5. refusals
@pytest.fixture(scope="module")
def cpu_net():
    from multimodal_vqvae_compression_audio_tactile_amd import build_proposed
    return build_proposed(None, rvq_books=2, rvq_embed=128, device="cpu")


def test_stream_sender_refusals_come_before_any_launch(cpu_net):
    """On a CPU-resident model nothing can have been launched: the checks come first."""
    from multimodal_vqvae_compression_audio_tactile_amd import MvqError, StreamSender, ops
    net = cpu_net
    for ptok in (3, 5, 32, 0):
        with pytest.raises(ValueError, match="does not divide"):
            net.stream_sender(packet_tok=ptok)
    with pytest.raises(ValueError, match="batch"):
        net.stream_sender(batch=0)
    tx = net.stream_sender(batch=2)
    assert isinstance(tx, StreamSender) and (tx.K, tx.nb, tx.tokens, tx.chunk, tx.finished) == (128, 2, 0, 0, False)
    assert tx.buf.shape == (4, 48 * 320) and tx.carry.shape == (2, 1024)
    assert net.stream_sender(books_use=1).nb == 1
    x = torch.zeros(2, 1, 5120)
    with pytest.raises(ValueError, match="batch"):
        tx.push(x[:1], x[:1])
    with pytest.raises(ValueError, match="batch"):
        tx.push(x, x[:1])
    with pytest.raises(ValueError, match="advance together"):
        tx.push(x, x[..., :2560])
    for n in (0, 100, 319, 321, 5440, 24000):
        with pytest.raises(ValueError, match="1 <= m <= 16"):
            tx.push(torch.zeros(2, 1, n), torch.zeros(2, 1, n))
    with pytest.raises(ValueError, match=r"\[B, 1, samples\]"):
        tx.push(torch.zeros(2, 5120), torch.zeros(2, 5120))
    with pytest.raises(ValueError, match="float"):
        tx.push(x.long(), x.long())
    with pytest.raises(ValueError, match="both|neither"):
        tx.finish(x)
    with pytest.raises(ValueError, match="advance together"):
        tx.finish(x, x[..., :100])
    assert (tx.tokens, tx.fill, tx.chunk) == (0, 0, 0) and not tx.buf.any()
    with ops.arith("bf16x6"):
        with pytest.raises(ValueError, match="arithmetic"):
            net.stream_sender()
        with pytest.raises(ValueError, match="arithmetic"):
            tx.push(x, x)
    tx.finished = True
    with pytest.raises(MvqError, match="after finish"):
        tx.push(x, x)
    with pytest.raises(MvqError, match="after finish"):
        tx.finish()
    # an item with no samples at all: nothing to send, and no launch
    tx = net.stream_sender(batch=2)
    pk, codes, info = tx.finish()
    assert pk == [[], []] and codes.shape == (2, 32, 0) and codes.dtype == torch.int64 and info == StreamInfo(128, 2, 0, 2)
    # the carried token of _ar_latents: of the right shape, and not without a recursion
    zt, z = torch.zeros(2, 1024, 16), torch.zeros(2, 1024)
    for bad in (z[:1], z.double(), torch.zeros(2, 1024, 1), torch.zeros(1024, 2).t()):
        with pytest.raises(MvqError, match="z_prev must be"):
            net._ar_latents(zt, zt, z_prev=bad)
        with pytest.raises(MvqError, match="z_last_out must be"):
            net._ar_latents(zt, zt, z_last_out=bad)
    with pytest.raises(MvqError, match="tactile_only"):
        net._ar_latents(None, zt, tactile_only=True, z_prev=z)


def test_sender_entry_points_check_their_arguments():
    import ctypes
    from multimodal_vqvae_compression_audio_tactile_amd import ProposedEval, _lib, ops
    assert callable(ProposedEval.stream_sender) and callable(getattr(ops, "stream_samples", None))
    lib = _lib.lib()
    for n in ("mvq_stream_samples_f32", "mvq_ar_latents_staged_carry_f32"):
        assert n in _lib.EXPORTS and hasattr(lib, n), n
    assert lib.mvq_abi_version() == 3
    # refused before any device access (no GPU here): (buf, fill, x_new, n, win, w, drop, cap, rows, stream)
    smp = lambda fill, n, w, drop, cap=15360, rows=2: lib.mvq_stream_samples_f32(None, fill, None, n, None, w, drop, cap, rows, None)
    for neg in ((-1, 320, 0, 0), (0, -320, 0, 0), (0, 320, -1, 0), (0, 320, 0, -1)):
        assert smp(*neg) == -1
    assert smp(0, 320, 0, 0, cap=-1) == -1 and smp(0, 320, 0, 0, rows=-1) == -1
    assert b"negative" in lib.mvq_last_error()
    assert smp(15361, 0, 0, 0) == -1 and b"capacity" in lib.mvq_last_error()                 # fill > cap
    assert smp(15360, 320, 0, 0) == -1 and b"capacity" in lib.mvq_last_error()               # fill + n - drop > cap
    assert smp(15360, 320, 0, 319) == -1
    assert smp(5120, 5120, 10241, 5120) == -1 and b"w = 10241" in lib.mvq_last_error()       # w > fill + n
    assert smp(5120, 5120, 10240, 10241) == -1 and b"drop = 10241" in lib.mvq_last_error()   # drop > fill + n
    assert smp(5120, 5120, 10240, 5120) == -1 and b"null" in lib.mvq_last_error()            # null pointers, non-empty shape
    assert smp(0, 320, 0, 0) == -1 and smp(320, 0, 320, 0) == -1 and smp(320, 0, 0, 320) == -1
    assert smp(5120, 5120, 10240, 5120, rows=0) == 0                                          # empty: 0 without a launch
    assert smp(5120, 0, 0, 0) == 0 and smp(0, 0, 0, 0) == 0
    # the carried staged loop shares the staged loop's checks
    carry = lib.mvq_ar_latents_staged_carry_f32
    assert carry(None, None, None, None, 0, None) == -1 and b"null argument" in lib.mvq_last_error()
    a = _lib.ArArgs()
    assert carry(ctypes.byref(a), None, None, None, 0, None) == 0                             # batch 0: nothing to do
    a.batch, a.t_lat, a.c_lat, a.c_ff, a.code_dim, a.heads, a.chunk, a.rvq_k = 1, 16, 1024, 2048, 96, 8, 16, 128
    assert carry(ctypes.byref(a), None, None, None, 0, None) == -1 and b"null tensor" in lib.mvq_last_error()
    a.c_lat = 512
    assert carry(ctypes.byref(a), None, None, None, 0, None) == -2
