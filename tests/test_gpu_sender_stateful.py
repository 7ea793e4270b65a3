"""-m gpu: the stateful streaming encoder -- the Snake stage-window kernel against torch indexing and the
conv epilogue's own Snake (dense and slots), Stack.encoder_stream_fwd piece by piece against encoder_fwd of the whole signal,
StreamSender(encoder="stateful") against the window mode push by push and against compress_packets / compress_packets_av, the
captured steady step, the pool, the link under loss.  Every comparison is an equality.  The stream plan keeps dense rows at every
batch size (it does not take encoder_fwd's virtually packed tail), so there is no batch threshold to cross."""
import numpy as np
import pytest
import torch

import sender_oracle as sn
import test_gpu_fec as tf
from multimodal_vqvae_compression_audio_tactile_amd import bitstream, stream
from test_gpu_sender import LENGTHS, _case, _channel, _check_session, _net, _run_sender, _seq
from test_gpu_sender_pool import OPENS, _drive, _patterns

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------- 1. the Snake stage-window kernel
# (h_in, n, h_out, cap, src_t, src_off, win_t)
WINDOWS = [
    (7, 16, 9, 12, 37, 5, 23),            # nothing aligned: the 4-byte path
    (7, 16, 9, 12, 37, 5, 26),            # ... with a zero tail of 3 columns
    (0, 16, 12, 12, 37, 5, 16),           # a new session: no tail read
    (12, 0, 12, 12, 37, 5, 12),           # nothing new: the tail alone
    (7, 16, 0, 12, 37, 5, 23),            # the finish: nothing kept
    (8, 16, 12, 12, 40, 4, 28),           # every count a multiple of 4: the 16-byte path, a zero tail of 4
    (5, 3000, 12, 12, 3010, 5, 3005),     # a row longer than a block's share (one block per row, 12 passes)
]


def _snake_ref(x, alpha):
    """The Snake the conv epilogues write: a 1x1 identity conv's dual output (y == x exactly, y2 = snake(y))."""
    from multimodal_vqvae_compression_audio_tactile_amd import ops
    C = x.shape[1]
    wp = ops.pack_conv1d(torch.eye(C, device=x.device).reshape(C, C, 1).contiguous())
    y, y2 = ops.conv1d(x.contiguous(), wp, C, 1, alpha_dual=alpha)
    assert torch.equal(y, x)
    return y2


def _window_case(dev, C, shape, slots, n_rows, seed):
    from multimodal_vqvae_compression_audio_tactile_amd import ops
    h_in, n, h_out, cap, src_t, src_off, win_t = shape
    B = n_rows if slots is None else len(slots)
    g = torch.Generator().manual_seed(seed)
    off = 8                                                             # the stage's tail starts 8 floats into a state row
    S = off + C * cap + 4
    state = torch.full((n_rows, S), float("nan"), device=dev)
    rows = list(range(B)) if slots is None else slots
    tails = torch.randn(B, C, cap, generator=g).to(dev)
    for i, r in enumerate(rows):
        state[r, off:off + C * cap].view(C, cap)[:, :h_in] = tails[i, :, :h_in]
    src = torch.randn(B, C, src_t, generator=g).to(dev)
    alpha = (0.5 + torch.rand(C, generator=g)).to(dev)
    before = state.clone()
    win, win_s = ops.stream_stage_window_snake(state, h_in, src, src_off, n, h_out, cap, alpha, tail_off=off, win_t=win_t, slots=slots)
    W = h_in + n
    full = torch.cat([tails[..., :h_in], src[..., src_off:src_off + n]], dim=-1)
    assert win.shape == win_s.shape == (B, C, win_t)
    assert torch.equal(win[..., :W], full) and not torch.isnan(win).any() and not torch.isnan(win_s).any()
    assert torch.equal(win_s[..., :W], _snake_ref(full, alpha)) if W else True
    for t in (win, win_s):                                              # the zero tail is +0 in both outputs
        assert not t[..., W:].any() and not torch.signbit(t[..., W:]).any()
    want = before.clone()
    for i, r in enumerate(rows):
        want[r, off:off + C * cap].view(C, cap)[:, :h_out] = full[i, :, W - h_out:]
    # NaN everywhere else -- unlisted rows, the floats around the tail, tail columns at and past max(h_in, h_out) -- is untouched
    assert torch.equal(state.view(torch.int32), want.view(torch.int32))
    assert torch.isnan(state[rows[0], :off]).all() and (h_out == cap or torch.isnan(state[rows[0], off:off + C * cap].view(C, cap)[:, max(h_in, h_out):]).all())


@pytest.mark.parametrize("C", [48, 128])
def test_snake_stage_window_equals_torch_indexing_dense(C, dev):
    for i, shape in enumerate(WINDOWS):
        _window_case(dev, C, shape, None, 3, 100 * C + i)


@pytest.mark.parametrize("C", [48, 128])
def test_snake_stage_window_slots_equals_torch_indexing(C, dev):
    for i, shape in enumerate(WINDOWS):
        _window_case(dev, C, shape, [4, 0, 2], 6, 200 * C + i)


def test_snake_stage_window_out_of_range_slot_reads_zeros_and_stores_nothing(dev):
    from multimodal_vqvae_compression_audio_tactile_amd import _lib, ops
    C, cap = 48, 12
    state = torch.full((3, C * cap), float("nan"), device=dev)
    state[1].view(C, cap)[:, :7] = 1.5
    before = state.clone()
    src = torch.randn(2, C, 37, device=dev)
    alpha = torch.ones(C, device=dev)
    sd = torch.tensor([1, 7], dtype=torch.int32, device=dev)           # slot 7 of 3: the kernel's own guard (the wrapper would refuse it)
    win, win_s = torch.empty(2, C, 23, device=dev), torch.empty(2, C, 23, device=dev)
    rc = _lib.lib().mvq_stream_stage_window_snake_slots_f32(state.data_ptr(), C * cap, sd.data_ptr(), 2, 3, 7, src.data_ptr(), 37, 5, 16, win.data_ptr(),
                                                            win_s.data_ptr(), alpha.data_ptr(), 23, 9, cap, C, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    assert torch.equal(win[1, :, :7], torch.zeros(C, 7, device=dev)) and torch.equal(win_s[1, :, :7], torch.zeros(C, 7, device=dev))
    assert torch.equal(win[1, :, 7:], src[1, :, 5:21]) and torch.equal(win[0, :, :7], torch.full((C, 7), 1.5, device=dev))
    assert torch.equal(state[[0, 2]].view(torch.int32), before[[0, 2]].view(torch.int32))
    assert torch.equal(state[1].view(C, cap)[:, :9], win[0, :, 14:])
    # the refusals of the entry point launch nothing
    L = _lib.lib()
    args = lambda **kw: [kw.get(k, v) for k, v in dict(tail=state.data_ptr(), stride=C * cap, h_in=7, src=src.data_ptr(), src_t=37, src_off=5, n=16,
                                                      win=win.data_ptr(), win_s=win_s.data_ptr(), alpha=alpha.data_ptr(), win_t=23, h_out=9, cap=cap,
                                                      batch=2, c=C, stream=None).items()]
    keep = state.clone()
    for kw, msg in ((dict(src_off=22), b"outside the source rows"), (dict(win_t=22), b"window rows"), (dict(h_out=13), b"exceed"),
                    (dict(win_s=None), b"null"), (dict(alpha=None), b"null"), (dict(stride=C * cap - 1), b"holds no")):
        assert L.mvq_stream_stage_window_snake_f32(*args(**kw)) == -1 and msg in L.mvq_last_error(), kw
    torch.cuda.synchronize()
    assert torch.equal(state.view(torch.int32), keep.view(torch.int32))


# ------------------------------------------------------------------------------------------------ 2. Stack.encoder_stream_fwd
_WHOLE = {}


def _whole(dev, B, L):
    """encoder_fwd of seeded signals, both encoders' stacks -- once per (B, L)."""
    if (B, L) not in _WHOLE:
        from multimodal_vqvae_compression_audio_tactile_amd import synth
        net = _net(dev)
        x = synth.tactile_segments(B, seed=L % 1000 + B, T=L).to(dev)
        _WHOLE[(B, L)] = (x, net.T_ENC.stack().encoder_fwd(x))
    return _WHOLE[(B, L)]


def _pieces(stack, state, x, cuts, slots=None):
    """Feed x in pieces that end at ``cuts`` (samples), the last one with last=True -> the emitted columns concatenated, and the
    global column range of every step."""
    out, spans, pos = [], [], 0
    for i, end in enumerate(cuts):
        last = i == len(cuts) - 1
        _, (t0, t1) = stack.encoder_stream_plan(pos, end - pos, last)
        z = stack.encoder_stream_fwd(state, x[..., pos:end].contiguous(), pos, last, slots=slots)
        assert z.shape[-1] == t1 - t0
        out.append(z)
        spans.append((t0, t1))
        pos = end
    return torch.cat(out, dim=-1), spans


def _session_cuts(L):
    """24 tokens, then 16 at a time, then the finish with whatever remains (nothing, when 320 | L and the chunks use it up)."""
    cuts = [c for c in range(24 * 320, L + 1, 16 * 320)]
    return cuts + [L]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("L", [320 * 11, 320 * 16, 320 * 37, 320 * 75, 320 * 40 - 137])
def test_stack_stream_fwd_equals_whole_signal_encode(L, B, dev):
    stack = _net(dev).T_ENC.stack()
    x, whole = _whole(dev, B, L)
    state = torch.full((B, stack.encoder_stream_state_floats()), float("nan"), device=dev)
    cuts = _session_cuts(L)
    got, spans = _pieces(stack, state, x, cuts)
    assert got.shape == whole.shape and torch.equal(got, whole)
    T = whole.shape[-1]
    assert [t1 - t0 for t0, t1 in spans[:-1]] == [16] * (len(cuts) - 1) and spans[-1][1] == T == stream.enc_tokens(L)


def test_stack_stream_fwd_any_piece_sizes_and_slots(dev):
    """Pieces of 5 / 16 / 1 / 9 tokens, repeated, three sessions on rows [4, 0, 2] of a NaN-filled state of six rows; and the audio
    encoder's stack with a finish that brings no samples."""
    net = _net(dev)
    for stack, L in ((net.T_ENC.stack(), 320 * 40 - 137), (net.A_ENC.stack(), 320 * 37)):
        x, _ = _whole(dev, 3, L)
        whole = stack.encoder_fwd(x)
        cuts, pos = [], 0
        for m in [5, 16, 1, 9] * 4:
            if pos + 320 * m > L:
                break
            pos += 320 * m
            cuts.append(pos)
        cuts.append(L)                                                  # 320 * 37: 31 tokens pushed + 6 more; the other: a ragged tail
        state = torch.full((6, stack.encoder_stream_state_floats()), float("nan"), device=dev)
        got, _ = _pieces(stack, state, x, cuts, slots=[4, 0, 2])
        assert torch.equal(got, whole)
        assert torch.isnan(state[[1, 3, 5]]).all()
        dense = torch.full((3, stack.encoder_stream_state_floats()), float("nan"), device=dev)
        got, _ = _pieces(stack, dense, x, [L, L])                       # everything in one push, then a finish without samples
        assert torch.equal(got, whole)


def test_stack_stream_fwd_refusals_launch_nothing(dev):
    from multimodal_vqvae_compression_audio_tactile_amd import _lib, ops
    stack = _net(dev).T_ENC.stack()
    L, S = _lib.lib(), stack.encoder_stream_state_floats()
    state = torch.full((2, S), float("nan"), device=dev)
    x = torch.zeros(2, 1, 7680, device=dev)
    z = torch.empty(2, 1024, 16, device=dev)
    nb = L.mvq_encoder_stream_workspace_bytes(stack.handle, 2, 0, 7680, 0)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    call = lambda z_len, ws_bytes: L.mvq_encoder_stream_fwd_f32(stack.handle, state.data_ptr(), None, 2, 2, x.data_ptr(), 7680, 0, 0, z.data_ptr(), z_len,
                                                               ws.data_ptr(), ws_bytes, torch.cuda.current_stream().cuda_stream)
    assert call(15, nb) == -1 and b"the step emits 16" in L.mvq_last_error()
    assert call(16, nb - 512) == -1 and b"workspace too small" in L.mvq_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(state).all()
    with pytest.raises(ValueError, match="state must be"):
        stack.encoder_stream_fwd(state[:, :-1], x, 0)
    with pytest.raises(ValueError, match="2 sessions, the state has 1"):
        stack.encoder_stream_fwd(state[:1], x, 0)
    with ops.arith("bf16x6"):
        with pytest.raises(ValueError, match="bf16x6"):
            stack.encoder_stream_fwd(state, x, 0)


# ----------------------------------------------------------------------------------------------------- 3. StreamSender
def _same(win_step, st_step):
    assert len(win_step) == len(st_step)
    for w, s in zip(win_step, st_step):
        if isinstance(w, torch.Tensor):
            assert w.shape == s.shape and w.dtype == s.dtype and torch.equal(w, s)
        else:
            assert w == s


@pytest.mark.parametrize("L", [LENGTHS[0], LENGTHS[4]])
@pytest.mark.parametrize("B", [1, 3, 9])
def test_stateful_sender_equals_window_mode_push_by_push(B, L, dev):
    net = _net(dev)
    ref = _case(dev, B, L)
    for pattern in (16, "mixed"):
        pushes = sn.split_pushes(L, pattern, seed=L + B)
        out_w, info_w = _run_sender(net.stream_sender(batch=B), ref[0], ref[1], pushes)
        tx = net.stream_sender(batch=B, encoder="stateful")
        out_s, info_s = _run_sender(tx, ref[0], ref[1], pushes)
        assert info_w == info_s and len(out_w) == len(out_s) and tx.encoder == "stateful" and tx.enc_state[0].shape[0] == B
        for w, s in zip(out_w, out_s):
            _same(w, s)
        _check_session(out_s, info_s, B, ref, pushes)                   # and so compress_packets, byte for byte


def test_stateful_sender_short_items_and_one_token_pushes(dev):
    net = _net(dev)
    # ... and 40 tokens as 16 + 8 + 16: the last push encodes every sample, so the finish flushes the stage tails alone
    for L, pushes in ((LENGTHS[2], [16]), (LENGTHS[3], [1] * 11), (LENGTHS[1], [1] * 37), (320 * 40, [16, 8, 16])):
        ref = _case(dev, 1, L)
        out, info = _run_sender(net.stream_sender(batch=1, encoder="stateful"), ref[0], ref[1], pushes)
        _check_session(out, info, 1, ref, pushes)


@pytest.mark.parametrize("B,L", [(1, 24000), (3, 12663)])
def test_stateful_sender_with_rate_audio_packets_and_fec(B, L, dev):
    net = _net(dev)
    a, t = tf._signals(dev, B, L)
    infos, pk, ainfos, apk, par, apar = net.compress_packets_av(a, t, rate=tf.RATE, audio_rate=tf.ARATE, fec=tf.FEC, audio_fec=tf.AFEC)
    pushes = sn.split_pushes(L, "mixed", seed=L + B)
    kw = dict(batch=B, rate=tf.RATE, audio="packets", audio_rate=tf.ARATE, fec=tf.FEC, audio_fec=tf.AFEC)
    out_w, infos_w = tf._run_sender(net.stream_sender(**kw), a, t, pushes, 2)
    out_s, infos_s = tf._run_sender(net.stream_sender(encoder="stateful", **kw), a, t, pushes, 2)
    assert infos_w == infos_s == (infos[0], ainfos[0]) and out_w == out_s
    for b in range(B):
        for k, want in enumerate((pk, apk, par, apar)):
            assert tf._cat(out_s, k, b) == want[b], (b, k)
    kw = dict(batch=B, rate=tf.RATE, fec=tf.FEC)                        # the audio codes as codes: (packets, codes, parity)
    out_w, info_w = tf._run_sender(net.stream_sender(**kw), a, t, pushes, 1)
    out_s, info_s = tf._run_sender(net.stream_sender(encoder="stateful", **kw), a, t, pushes, 1)
    assert info_w == info_s
    for w, s in zip(out_w, out_s):
        _same(w, s)


def test_stateful_sender_graph_replays_the_steady_step(dev):
    from multimodal_vqvae_compression_audio_tactile_amd import synth
    net = _net(dev)
    L = 320 * 96
    a, t = synth.audio_segments(1, seed=96, T=L).to(dev), synth.tactile_segments(1, seed=96, T=L).to(dev)
    eager, info_e = _run_sender(net.stream_sender(batch=1), a, t, [16] * 6)             # the window mode, eagerly
    txg = net.stream_sender(batch=1, graph=True, encoder="stateful")
    graphed, info_g = _run_sender(txg, a, t, [16] * 6)
    assert txg._g is not None and isinstance(txg._g[0], torch.cuda.CUDAGraph) and info_e == info_g
    assert len(eager) == len(graphed) == 7
    steady = [step[0][0] for step in graphed[2:6]]                                      # chunks 1..4: four runs of the one graph
    assert all(len(p) == 8 for p in steady) and len({b"".join(x[9:] for x in p) for p in steady}) == 4
    for i, (e, g) in enumerate(zip(eager, graphed)):
        assert e[0] == g[0] and torch.equal(e[1], g[1]), i
    infos, pk, aud = net.compress_packets(a, t)
    assert sum((step[0][0] for step in graphed), []) == pk[0] and info_g == infos[0]
    assert torch.equal(torch.cat([s[1] for s in graphed], dim=2).cpu(), torch.from_numpy(bitstream.unpack_indices(aud[0])[0])[None])


# ---------------------------------------------------------------------------------------------------------------- 4. pool
def test_stateful_pool_equals_solo_sessions_and_the_window_pool(dev):
    net = _net(dev)
    refs = [_case(dev, 1, L) for L in LENGTHS]
    patterns = _patterns()
    pool = net.stream_sender_pool(slots=4, encoder="stateful")
    for s in pool.enc_state:
        s.fill_(float("nan"))                                                           # open() clears nothing: a new session reads no tail
    outs, infos, slot, ticks = _drive(pool, [r[:2] for r in refs], patterns, OPENS)
    outs_w, infos_w, _, ticks_w = _drive(net.stream_sender_pool(slots=4), [r[:2] for r in refs], patterns, OPENS)
    assert pool.active == () and pool.free == 4 and slot[4] == min(slot[1], slot[2])    # the fifth session reuses a used slot
    members = lambda tk: [sorted(g.key[:1] + g.sids for g in groups) for groups, _ in tk]
    assert members(ticks) == members(ticks_w)                                           # the same sessions share launches in both modes
    assert any(len(g.sids) > 1 and g.hi > g.lo for groups, _ in ticks for g in groups)
    for i, ref in enumerate(refs):
        _check_session(outs[i], infos[i], 1, ref, patterns[i])
        assert infos[i] == infos_w[i] and len(outs[i]) == len(outs_w[i])
        for w, s in zip(outs_w[i], outs[i]):
            assert w[0] == s[0] and torch.equal(w[1], s[1])
        a, t = ref[:2]                                                                  # a solo stateful session, step by step
        tx, pos = net.stream_sender(batch=1, encoder="stateful"), 0
        for j, m in enumerate(patterns[i]):
            pk, codes = tx.push(a[..., pos:pos + 320 * m], t[..., pos:pos + 320 * m])
            pos += 320 * m
            assert outs[i][j][0] == pk and torch.equal(outs[i][j][1], codes), (i, j)
        pk, codes, info = tx.finish(a[..., pos:], t[..., pos:]) if pos < a.shape[-1] else tx.finish()
        assert outs[i][-1][0] == pk and torch.equal(outs[i][-1][1], codes) and infos[i] == info


# ---------------------------------------------------------------------------------------------------------- 5. full link
@pytest.mark.parametrize("name", ["alternating", "thin1"])
def test_stateful_sender_into_stateful_receiver_equals_the_whole_item_link(name, dev):
    net = _net(dev)
    B, L = 2, 24000
    a, t, infos, pk, codes = _case(dev, B, L)
    info = infos[0]
    aud = [bitstream.pack_indices(codes[b].numpy(), 1024) for b in range(B)]
    want = net.decompress_packets(infos, [_channel(pk[b], b, name, info) for b in range(B)], aud)[0]
    tx, rx = net.stream_sender(batch=B, encoder="stateful"), net.stream_receiver(512, 8, batch=B, decoder="stateful")
    ys, pend_pk, pend_codes = [], [[] for _ in range(B)], []

    def relay(step, last):
        for b in range(B):
            pend_pk[b] += _channel(step[0][b], b, name, info)
        pend_codes.append(step[1])
        have = torch.cat(pend_codes, dim=2)
        while have.shape[2] >= 16:
            lo_seq = rx.tokens // 2
            ys.append(rx.push([[p for p in pend_pk[b] if lo_seq <= _seq(p) < lo_seq + 8] for b in range(B)], have[..., :16]))
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
