"""-m gpu: the streaming sender on the device -- the sample-state kernel against torch.cat / slicing, _ar_latents(z_prev=) chunk by
chunk against the whole-item call in both of its forms, StreamSender end to end against compress_packets on the same signals, the
captured steady step, the sender feeding the streaming receiver over a lossy channel, and the refusals.
Every comparison is an equality."""
import numpy as np
import pytest
import torch

import lossy_oracle as lo
import sender_oracle as sn
from multimodal_vqvae_compression_audio_tactile_amd import bitstream, packets, stream
from multimodal_vqvae_compression_audio_tactile_amd.packets import StreamInfo

pytestmark = pytest.mark.gpu

_NETS, _REF = {}, {}
GUARD = 64
CAP = 48 * 320


def _net(dev, books=8, K=512, seed=7):
    """The b8_k512 model of golden_inputs.PE_CASES, as tests/test_gpu_stream.py builds it."""
    import golden_inputs as gi
    assert gi.PE_CASES["b8_k512"][:2] == (books, K) and gi.PE_CASES["b8_k512"][4] == seed
    if (books, K, seed) not in _NETS:
        from multimodal_vqvae_compression_audio_tactile_amd import build_proposed
        _NETS[(books, K, seed)] = build_proposed(gi.model_state(seed, books, K), rvq_books=books, rvq_embed=K, device=dev)
    return _NETS[(books, K, seed)]


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------------ 1. stream_samples
# (fill, n, w, drop)
SAMPLE_SHAPES = [
    (2560, 1600, 0, 0),              # a pure append
    (0, 7680, 7680, 2560),           # the first emit: 24 tokens in, the window is all of them, 8 tokens dropped
    (5120, 5120, 10240, 5120),       # the steady emit: 16 tokens onto 16 held ones
    (7680, 5120, 10240, 5120),       # ... onto 24 (every push 16 tokens): the window is not all of the samples in hand
    (9920, 320, 10240, 5120),        # a 1-token push that completes a chunk
    (12000, 3000, 100, 7),           # a shift by 7: every tile overlaps itself; nothing aligned
    (4097, 1, 4098, 1),              # one sample, a shift by one across the first tile's edge
    (15040, 320, 15360, 0),          # the append that fills the buffer
    (15360, 5120, 20480, 5120),      # a full buffer moved on and full again; fill + n exceeds the capacity
    (5120, 2423, 7543, 7543),        # finish: everything out, nothing kept
]


@pytest.mark.parametrize("R", [2, 6])
def test_stream_samples_equals_cat_and_slicing(R, dev):
    from multimodal_vqvae_compression_audio_tactile_amd import _lib, ops
    g = torch.Generator(device="cpu").manual_seed(R)
    for fill, n, w, drop in SAMPLE_SHAPES:
        buf0 = torch.randn(R, CAP, generator=g).to(dev)
        x = torch.randn(R, n, generator=g).to(dev)
        v = torch.cat([buf0[:, :fill], x], dim=1)
        keep = fill + n - drop
        want_buf = buf0.clone()
        want_buf[:, :keep] = v[:, drop:]
        buf = buf0.clone()
        win = ops.stream_samples(buf, fill, x, w, drop)
        assert win.shape == (R, w) and win.is_contiguous()
        assert torch.equal(win, v[:, :w]) and torch.equal(buf, want_buf), (fill, n, w, drop)
        # the C entry point into NaN-filled outputs with a guard band behind them: every element written, none beyond, and the
        # buffer columns past the new fill left alone
        out = torch.full((R * w + GUARD,), float("nan"), device=dev)
        bbuf = torch.cat([buf0.reshape(-1), torch.full((GUARD,), float("nan"), device=dev)])
        rc = _lib.lib().mvq_stream_samples_f32(bbuf.data_ptr(), fill, x.data_ptr(), n, out.data_ptr(), w, drop, CAP, R, _stream())
        assert rc == 0
        assert torch.equal(out[:R * w].view(R, w), v[:, :w]) and bool(torch.isnan(out[R * w:]).all()), (fill, n, w, drop)
        assert torch.equal(bbuf[:R * CAP].view(R, CAP), want_buf) and bool(torch.isnan(bbuf[R * CAP:]).all()), (fill, n, w, drop)


def test_stream_samples_refusals_launch_nothing(dev):
    from multimodal_vqvae_compression_audio_tactile_amd import MvqError, _lib, ops
    lib = _lib.lib()
    buf = torch.full((2, CAP), 3.0, device=dev)
    x = torch.ones(2, 5120, device=dev)
    win = torch.full((2, 10240), float("nan"), device=dev)
    call = lambda fill, n, w, drop, cap=CAP, R=2, bp=buf.data_ptr(), xp=x.data_ptr(), wp=win.data_ptr(): \
        lib.mvq_stream_samples_f32(bp, fill, xp, n, wp, w, drop, cap, R, _stream())
    assert call(5120, 5120, 10241, 5120) == -1 and b"w = 10241" in lib.mvq_last_error()
    assert call(5120, 5120, 10240, 10241) == -1 and b"drop = 10241" in lib.mvq_last_error()
    assert call(CAP + 1, 0, 0, 0) == -1 and call(CAP, 320, 0, 319) == -1 and b"capacity" in lib.mvq_last_error()
    for bad in ((-1, 5120, 0, 0), (5120, -1, 0, 0), (5120, 5120, -1, 0), (5120, 5120, 0, -1)):
        assert call(*bad) == -1
    assert call(5120, 5120, 10240, 5120, cap=-1) == -1 and call(5120, 5120, 10240, 5120, R=-1) == -1
    assert call(5120, 5120, 10240, 5120, bp=None) == -1 and call(5120, 5120, 10240, 5120, xp=None) == -1 \
        and call(5120, 5120, 10240, 5120, wp=None) == -1
    assert b"null" in lib.mvq_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(win).all()) and bool((buf == 3.0).all())                    # nothing ran
    assert call(5120, 5120, 10240, 5120, R=0) == 0 and call(5120, 0, 0, 0) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(win).all()) and bool((buf == 3.0).all())
    with pytest.raises(MvqError):
        ops.stream_samples(buf, 5120, x, 10241, 0)
    with pytest.raises(MvqError):
        ops.stream_samples(buf[:1], 5120, x, 0, 0)
    with pytest.raises(MvqError):
        ops.stream_samples(buf.cpu(), 5120, x, 0, 0)
    with pytest.raises(MvqError):
        ops.stream_samples(buf[:, :10240], 5120, x, 0, 0)                               # not contiguous: the pitch is the capacity
    assert bool((buf == 3.0).all())


# ------------------------------------------------------------------------------------------------- 2. the carried token
@pytest.mark.parametrize("Tlat", [75, 37])
@pytest.mark.parametrize("B", [3, 9])
def test_ar_latents_chunk_by_chunk_equals_the_whole_item(B, Tlat, dev):
    net = _net(dev)
    g = torch.Generator(device="cpu").manual_seed(B * 100 + Tlat)
    qa = (0.5 * torch.randn(B, 1024, Tlat, generator=g)).to(dev)
    zt = (0.5 * torch.randn(B, 1024, Tlat, generator=g)).to(dev)
    assert net._ar_one_call_mode(zt, net.vq.stacked()) == ("staged" if B <= 8 else None)  # B = 3: one host call; B = 9: the Python loop
    want_z, _, want_idx = net._ar_latents(qa, zt, want_indices=True)
    assert want_idx.shape == (8, B, Tlat)
    carry = torch.zeros(B, 1024, device=dev)
    zs, ids = [], []
    for s in range(0, Tlat, 16):
        e = min(Tlat, s + 16)
        z, _, idx = net._ar_latents(qa[..., s:e].contiguous(), zt[..., s:e].contiguous(), want_indices=True,
                                    z_prev=carry if s else None, z_last_out=carry)
        assert torch.equal(carry, z[..., -1])
        zs.append(z)
        ids.append(idx)
    assert torch.equal(torch.cat(ids, dim=2), want_idx) and torch.equal(torch.cat(zs, dim=2), want_z)
    # two pieces of several chunks each, and a zero z_prev is what chunk 0 is fed today
    carry.zero_()
    cut = 32
    z0, _, i0 = net._ar_latents(qa[..., :cut].contiguous(), zt[..., :cut].contiguous(), want_indices=True, z_prev=carry, z_last_out=carry)
    z1, _, i1 = net._ar_latents(qa[..., cut:].contiguous(), zt[..., cut:].contiguous(), want_indices=True, z_prev=carry, z_last_out=carry)
    assert torch.equal(torch.cat([z0, z1], dim=2), want_z) and torch.equal(torch.cat([i0, i1], dim=2), want_idx)
    assert torch.equal(carry, want_z[..., -1])


# ------------------------------------------------------------------------------------------------------- 3. end to end
LENGTHS = [24000, 320 * 37, 5120, 320 * 11, 320 * 40 - 137]


def _case(dev, B, L):
    """compress_packets on seeded inputs of L samples -- once per (B, L)."""
    if (B, L) not in _REF:
        from multimodal_vqvae_compression_audio_tactile_amd import synth
        net = _net(dev)
        a, t = synth.audio_segments(B, seed=L % 1000 + B, T=L).to(dev), synth.tactile_segments(B, seed=L % 1000 + B, T=L).to(dev)
        infos, pk, aud = net.compress_packets(a, t)
        codes = torch.from_numpy(np.stack([bitstream.unpack_indices(p)[0] for p in aud]))
        T = stream.enc_tokens(L)
        assert tuple(infos[0]) == (512, 8, T, 2) and codes.shape == (B, 32, T)
        _REF[(B, L)] = (a, t, infos, pk, codes)
    return _REF[(B, L)]


def _run_sender(tx, a, t, pushes):
    """Feed a StreamSender the pushes (tokens each), then finish with the rest -> (per-step outputs, StreamInfo)."""
    out, pos = [], 0
    for m in pushes:
        out.append(tx.push(a[..., pos:pos + 320 * m], t[..., pos:pos + 320 * m]))
        pos += 320 * m
    pk, codes, info = tx.finish(a[..., pos:], t[..., pos:]) if pos < a.shape[-1] else tx.finish()
    out.append((pk, codes))
    return out, info


def _check_session(out, info, B, ref, pushes):
    a, t, infos, pk, codes = ref
    T = infos[0].T
    assert info == infos[0]
    for b in range(B):
        assert sum((step[0][b] for step in out), []) == pk[b], b                      # byte for byte, in order
    got = torch.cat([step[1] for step in out], dim=2)
    assert got.dtype == torch.int64 and torch.equal(got.cpu(), codes)
    # what each step emitted is what the schedule says
    steps = stream.sender_schedule(T, pushes)
    assert [step[1].shape[2] for step in out] == [min(16 * c1, T) - 16 * c0 if c1 > c0 else 0 for _, _, c0, c1, _ in steps]


@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("B", [1, 3, 9])
def test_stream_sender_equals_compress_packets(B, L, dev):
    net = _net(dev)
    ref = _case(dev, B, L)
    for pattern in (16, 8, "mixed"):
        pushes = sn.split_pushes(L, pattern, seed=L + B)
        tx = net.stream_sender(batch=B)
        out, info = _run_sender(tx, ref[0], ref[1], pushes)
        _check_session(out, info, B, ref, pushes)
        assert tx.finished and tx.chunk == -(-info.T // 16) and tx._g is None


def test_stream_sender_one_token_pushes(dev):
    net = _net(dev)
    ref = _case(dev, 1, 24000)
    out, info = _run_sender(net.stream_sender(batch=1), ref[0], ref[1], [1] * 75)
    _check_session(out, info, 1, ref, [1] * 75)
    assert [i for i, step in enumerate(out[:-1]) if step[0][0]] == [23, 39, 55, 71]     # the push that brings token 16c + 24


def test_stream_sender_other_packet_sizes_and_fewer_books(dev):
    net = _net(dev)
    a, t = _case(dev, 3, 320 * 37)[:2]
    for ptok, use in ((4, None), (16, 3), (1, 8)):
        infos, pk, aud = net.compress_packets(a, t, books_use=use, packet_tok=ptok)
        out, info = _run_sender(net.stream_sender(packet_tok=ptok, batch=3, books_use=use), a, t, [16, 16])
        assert info == infos[0] and info.nb == (8 if use is None else use)
        for b in range(3):
            assert sum((step[0][b] for step in out), []) == pk[b]


# --------------------------------------------------------------------------------------------------------------- 4. graph
def test_stream_sender_graph_replays_the_steady_step(dev):
    from multimodal_vqvae_compression_audio_tactile_amd import synth
    net = _net(dev)
    L = 320 * 96
    a, t = synth.audio_segments(1, seed=96, T=L).to(dev), synth.tactile_segments(1, seed=96, T=L).to(dev)
    eager, info_e = _run_sender(net.stream_sender(batch=1), a, t, [16] * 6)
    txg = net.stream_sender(batch=1, graph=True)
    graphed, info_g = _run_sender(txg, a, t, [16] * 6)
    assert txg._g is not None and isinstance(txg._g[0], torch.cuda.CUDAGraph)
    assert len(eager) == len(graphed) == 7 and info_e == info_g == StreamInfo(512, 8, 96, 2)
    steady = [step[0][0] for step in eager[2:6]]                        # chunks 1..4: four runs of the one graph
    assert all(len(p) == 8 for p in steady) and len({b"".join(x[9:] for x in p) for p in steady}) == 4
    for i, (e, g) in enumerate(zip(eager, graphed)):
        assert e[0] == g[0] and torch.equal(e[1], g[1]), i
    infos, pk, aud = net.compress_packets(a, t)
    assert sum((step[0][0] for step in graphed), []) == pk[0] and info_g == infos[0]
    assert torch.equal(torch.cat([s[1] for s in graphed], dim=2).cpu(), torch.from_numpy(bitstream.unpack_indices(aud[0])[0])[None])


# ----------------------------------------------------------------------------------------------------------- 5. full link
def _seq(pkt):
    return int.from_bytes(bytes(pkt)[3:7], "little")


def _channel(pk_item, b, name, info):
    """The packets of one item after the named loss pattern of tests/lossy_oracle.py (per packet: dropped, thinned or whole)."""
    v = lo.loss_pattern(name, b + 1, info.T, info.nb, info.packet_tok)[b]
    out = []
    for p in pk_item:
        t0 = _seq(p) * info.packet_tok
        have = int(v[t0:t0 + info.packet_tok].min())
        if have == 0:
            continue
        out.append(p if have >= info.nb else packets.thin(p, have, info))
    return out


@pytest.mark.parametrize("name", ["alternating", "thin1", "tok15"])
def test_stream_sender_into_stream_receiver_equals_the_whole_item_link(name, dev):
    net = _net(dev)
    B, L = 2, 24000
    a, t, infos, pk, codes = _case(dev, B, L)
    info = infos[0]
    aud = [bitstream.pack_indices(codes[b].numpy(), 1024) for b in range(B)]
    want = net.decompress_packets(infos, [_channel(pk[b], b, name, info) for b in range(B)], aud)[0]
    tx, rx = net.stream_sender(batch=B), net.stream_receiver(512, 8, batch=B)
    ys, pend_pk, pend_codes = [], [[] for _ in range(B)], []

    def relay(step, last):
        """What the sender emitted goes through the channel and into the receiver, one 16-token chunk at a time."""
        for b in range(B):
            pend_pk[b] += _channel(step[0][b], b, name, info)
        pend_codes.append(step[1])
        have = torch.cat(pend_codes, dim=2)
        while have.shape[2] >= 16:
            lo_seq = rx.tokens // 2
            mine = [[p for p in pend_pk[b] if lo_seq <= _seq(p) < lo_seq + 8] for b in range(B)]
            ys.append(rx.push(mine, have[..., :16]))
            have = have[..., 16:]
        pend_codes[:] = [have]
        if last:
            lo_seq = rx.tokens // 2
            tail = [[p for p in pend_pk[b] if _seq(p) >= lo_seq] for b in range(B)]
            ys.append(rx.finish(tail, have) if have.shape[2] else rx.finish())

    pos = 0
    for m in sn.split_pushes(L, "mixed", seed=3):
        relay(tx.push(a[..., pos:pos + 320 * m], t[..., pos:pos + 320 * m]), False)
        pos += 320 * m
    fpk, fcodes, finfo = tx.finish(a[..., pos:], t[..., pos:]) if pos < L else tx.finish()
    assert finfo == info
    relay((fpk, fcodes), True)
    got = torch.cat(ys, dim=-1)
    assert got.shape == want.shape == (B, 1, 320 * 75 - 8) and torch.equal(got, want)


# ----------------------------------------------------------------------------------------------------------- 6. refusals
def test_stream_sender_refusals_on_the_device(dev):
    from multimodal_vqvae_compression_audio_tactile_amd import MvqError, ops
    net = _net(dev)
    with pytest.raises(ValueError, match="does not divide"):
        net.stream_sender(packet_tok=3)
    tx = net.stream_sender(batch=2)
    x = torch.zeros(2, 1, 5120, device=dev)
    with pytest.raises(ValueError, match="batch"):
        tx.push(x[:1], x[:1])
    with pytest.raises(ValueError, match="advance together"):
        tx.push(x, x[..., :320])
    with pytest.raises(ValueError, match="1 <= m <= 16"):
        tx.push(x[..., :100], x[..., :100])
    with pytest.raises(ValueError, match="1 <= m <= 16"):
        tx.push(torch.zeros(2, 1, 5440, device=dev), torch.zeros(2, 1, 5440, device=dev))
    with ops.arith("f16x3"):
        with pytest.raises(ValueError, match="arithmetic"):
            tx.push(x, x)
    assert (tx.tokens, tx.fill, tx.chunk) == (0, 0, 0) and not tx.buf.any() and not tx.carry.any()      # nothing ran
    pk, codes = tx.push(x, x)
    assert pk == [[], []] and codes.shape == (2, 32, 0) and tx.tokens == 16
    pk, codes, info = tx.finish()
    assert [len(p) for p in pk] == [8, 8] and codes.shape == (2, 32, 16) and info == StreamInfo(512, 8, 16, 2)
    with pytest.raises(MvqError, match="after finish"):
        tx.push(x, x)
    with pytest.raises(MvqError, match="after finish"):
        tx.finish()
    zt, z = torch.zeros(2, 1024, 16, device=dev), torch.zeros(2, 1024, device=dev)
    with pytest.raises(MvqError, match="z_prev must be"):
        net._ar_latents(zt, zt, z_prev=z.cpu())
    with pytest.raises(MvqError, match="tactile_only"):
        net._ar_latents(None, zt, tactile_only=True, z_last_out=z)
