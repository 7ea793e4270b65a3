"""-m gpu: the stateful streaming decoder -- the stage-window kernel against torch indexing (dense and
slots), Stack.decoder_stream_fwd piece by piece against decoder_fwd of the whole latent, StreamReceiver(decoder="stateful")
against the window mode call by call and against the whole-item receivers, the captured steady step, the pool, the refusals.
Every comparison is an equality.  From 32 sessions on the stream plan keeps decoder_fwd's packed latent-rate head; batches of 32
and 35 engage it.  The model, the items and their loss patterns are those of
tests/test_gpu_stream.py, tests/test_gpu_fec.py and tests/test_gpu_audio_conceal.py."""
import numpy as np
import pytest
import torch

from multimodal_vqvae_compression_audio_tactile_amd import bitstream, packets, stream
from multimodal_vqvae_compression_audio_tactile_amd.packets import StreamInfo
from test_gpu_stream import _case, _net, _run_session, _seq, _stream, _whole

pytestmark = pytest.mark.gpu

_REF = {}
NAN = float("nan")


def _bits(x):
    return x.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------------- 1. the kernel
# (h_in, n, h_out, cap, src_t, src_off, tail_off, win_t): the unaligned source slice the stages see; h_in = 0 (a new session);
# n = 0 (a flush); h_out = h_in + n; h_out = 0 (the last step); a zero tail behind the window; every count a multiple of 4 (the
# 16-byte path); a window longer than a block's share (one row per block)
STAGE_SHAPES = [(12, 16, 12, 12, 37, 5, 3, None), (0, 16, 12, 12, 37, 5, 3, None), (12, 0, 12, 12, 37, 5, 3, None),
                (4, 8, 12, 12, 37, 5, 3, None), (12, 16, 0, 12, 37, 5, 3, None), (9, 12, 7, 12, 37, 5, 0, 24),
                (8, 16, 8, 12, 40, 4, 8, None), (8, 16, 8, 12, 40, 4, 8, 28), (20, 2200, 20, 20, 2300, 53, 4, None)]


def _stage_case(C, G, rows, shape, seed, dev):
    h_in, n, h_out, cap, src_t, src_off, tail_off, win_t = shape
    g = torch.Generator(device="cpu").manual_seed(seed)
    stride = (tail_off + C * cap + 7) // 4 * 4
    state0 = torch.randn(rows, stride, generator=g).to(dev)
    src = torch.randn(G, C, src_t, generator=g).to(dev)
    return state0, src, stride


def _stage_want(state0, src, sess, C, shape):
    h_in, n, h_out, cap, src_t, src_off, tail_off, win_t = shape
    G, W = src.shape[0], h_in + n
    wt = W if win_t is None else win_t
    tails = state0[sess][:, tail_off:tail_off + C * cap].reshape(G, C, cap)
    win = torch.cat([tails[..., :h_in], src[..., src_off:src_off + n], torch.zeros(G, C, wt - W, device=src.device)], dim=2)
    tails = tails.clone()
    tails[..., :h_out] = win[..., W - h_out:W]
    state = state0.clone()
    state[sess, tail_off:tail_off + C * cap] = tails.reshape(G, C * cap)
    return win, state


@pytest.mark.parametrize("C", [48, 96])
def test_stage_window_equals_torch_indexing_dense(C, dev):
    from multimodal_vqvae_compression_audio_tactile_amd import ops
    G = 3
    for i, shape in enumerate(STAGE_SHAPES):
        h_in, n, h_out, cap, src_t, src_off, tail_off, win_t = shape
        state0, src, stride = _stage_case(C, G, G, shape, 10 * C + i, dev)
        # NaN in the tail columns at and past h_in: never read into the window, and left alone past h_out
        tv = state0[:, tail_off:tail_off + C * cap].view(G, C, cap)
        tv[..., h_in:] = NAN
        want_win, want_state = _stage_want(state0, src, list(range(G)), C, shape)
        state = state0.clone()
        win = ops.stream_stage_window(state, h_in, src, src_off, n, h_out, cap, tail_off=tail_off, win_t=win_t)
        if h_in + n == 0:
            continue
        assert win.shape == want_win.shape and not bool(torch.isnan(win).any()), shape
        assert torch.equal(win, want_win) and torch.equal(_bits(state), _bits(want_state)), shape


@pytest.mark.parametrize("C", [48, 96])
def test_stage_window_slots_equals_torch_indexing(C, dev):
    from multimodal_vqvae_compression_audio_tactile_amd import ops
    slots, rows = [4, 0, 2], 5
    for i, shape in enumerate(STAGE_SHAPES):
        h_in, n, h_out, cap, src_t, src_off, tail_off, win_t = shape
        state0, src, stride = _stage_case(C, 3, rows, shape, 20 * C + i, dev)
        state0[[1, 3]] = NAN                                                 # the unlisted slots: neither read nor changed
        tv = state0[:, tail_off:tail_off + C * cap].view(rows, C, cap)
        tv[..., h_in:] = NAN
        want_win, want_state = _stage_want(state0, src, slots, C, shape)
        state = state0.clone()
        win = ops.stream_stage_window_slots(state, slots, h_in, src, src_off, n, h_out, cap, tail_off=tail_off, win_t=win_t)
        assert win.shape == want_win.shape and not bool(torch.isnan(win).any()), shape
        assert torch.equal(win, want_win) and torch.equal(_bits(state), _bits(want_state)), shape
        # the dense kernel on the gathered rows gives the same window
        dense = state0[slots].contiguous()
        assert torch.equal(ops.stream_stage_window(dense, h_in, src, src_off, n, h_out, cap, tail_off=tail_off, win_t=win_t), win)
        assert torch.equal(_bits(dense), _bits(want_state[slots]))


def test_stage_window_packed_rows_equal_torch_indexing(dev):
    """src_seg / win_seg > 1: item g is segment g % seg of row g // seg -- read from packed rows, written into packed rows, a group
    that does not fill its last row, dense and slots."""
    from multimodal_vqvae_compression_audio_tactile_amd import _lib
    lib = _lib.lib()
    C, G, seg, cap, h_in, n, h_out, src_per, src_off, win_per, rows = 48, 5, 4, 12, 12, 16, 12, 28, 5, 32, 7
    Gp = (G + seg - 1) // seg
    g = torch.Generator(device="cpu").manual_seed(5)
    slots = [6, 0, 3, 2, 5]
    sd = torch.tensor(slots, dtype=torch.int32, device=dev)
    for use_slots in (False, True):
        state0 = torch.randn(rows, C * cap, generator=g).to(dev)
        src = torch.randn(Gp, C, seg * src_per, generator=g).to(dev)
        sess = slots if use_slots else list(range(G))
        if use_slots:
            state0[[1, 4]] = NAN
        win = torch.full((Gp, C, seg * win_per), NAN, device=dev)
        want_win, want_state = win.clone(), state0.clone()
        for i, s_ in enumerate(sess):
            r, k = divmod(i, seg)
            t0 = state0[s_].view(C, cap)
            w = torch.cat([t0[:, :h_in], src[r, :, k * src_per + src_off:k * src_per + src_off + n], torch.zeros(C, win_per - h_in - n, device=dev)], 1)
            want_win[r, :, k * win_per:(k + 1) * win_per] = w
            want_state[s_].view(C, cap)[:, :h_out] = w[:, h_in + n - h_out:h_in + n]
        state = state0.clone()
        if use_slots:
            rc = lib.mvq_stream_stage_window_slots_f32(state.data_ptr(), C * cap, sd.data_ptr(), G, rows, h_in, src.data_ptr(), src_per, seg, src_off, n,
                                                       win.data_ptr(), win_per, seg, h_out, cap, C, _stream())
        else:
            rc = lib.mvq_stream_stage_window_f32(state.data_ptr(), C * cap, h_in, src.data_ptr(), src_per, seg, src_off, n, win.data_ptr(), win_per, seg,
                                                 h_out, cap, G, C, _stream())
        assert rc == 0
        assert torch.equal(_bits(win), _bits(want_win)) and torch.equal(_bits(state), _bits(want_state))      # spare segments untouched


def test_stage_window_refusals_launch_nothing(dev):
    from multimodal_vqvae_compression_audio_tactile_amd import MvqError, _lib, ops
    lib = _lib.lib()
    C, cap = 48, 12
    state = torch.full((2, C * cap), 3.0, device=dev)
    src = torch.ones(2, C, 37, device=dev)
    win = torch.full((2, C, 28), NAN, device=dev)
    sd = torch.tensor([1, 0], dtype=torch.int32, device=dev)

    def call(h_in=12, n=16, h_out=12, src_t=37, src_off=5, win_t=28, cap=cap, B=2, C=C, stride=C * cap, tp=state.data_ptr(),
             sp=src.data_ptr(), wp=win.data_ptr(), slots=False, src_seg=1, win_seg=1):
        if slots:
            return lib.mvq_stream_stage_window_slots_f32(tp, stride, sd.data_ptr(), B, 2, h_in, sp, src_t, src_seg, src_off, n, wp, win_t, win_seg,
                                                         h_out, cap, C, _stream())
        return lib.mvq_stream_stage_window_f32(tp, stride, h_in, sp, src_t, src_seg, src_off, n, wp, win_t, win_seg, h_out, cap, B, C, _stream())

    for slots in (False, True):
        assert call(h_in=2, h_out=19, cap=20, stride=C * 20, slots=slots) == -1 and b"exceeds h_in + n" in lib.mvq_last_error()
        assert call(h_in=13, slots=slots) == -1 and call(h_out=13, slots=slots) == -1            # past the capacity
        assert call(src_off=22, slots=slots) == -1 and b"outside the source rows" in lib.mvq_last_error()
        assert call(win_t=27, slots=slots) == -1 and call(stride=C * cap - 1, slots=slots) == -1
        assert call(src_seg=0, slots=slots) == -1 and call(win_seg=0, slots=slots) == -1 and call(win_seg=65, slots=slots) == -1
        for bad in (dict(h_in=-1), dict(n=-1), dict(h_out=-1), dict(src_t=-1), dict(src_off=-1), dict(win_t=-1), dict(cap=-1), dict(B=-1),
                    dict(C=-1)):
            assert call(slots=slots, **bad) == -1, bad
        assert call(tp=None, slots=slots) == -1 and call(sp=None, slots=slots) == -1 and call(wp=None, slots=slots) == -1
        assert b"null" in lib.mvq_last_error()
        assert call(B=0, slots=slots) == 0 and call(h_in=0, n=0, h_out=0, slots=slots) == 0       # nothing to do: no launch
    assert lib.mvq_stream_stage_window_slots_f32(state.data_ptr(), C * cap, sd.data_ptr(), 3, 2, 12, src.data_ptr(), 37, 1, 5, 16, win.data_ptr(), 28, 1,
                                                 12, cap, C, _stream()) == -1                      # a group larger than the pool
    with pytest.raises(MvqError, match="listed twice"):
        ops.stream_stage_window_slots(state, [1, 1], 12, src, 5, 16, 12, cap)
    with pytest.raises(MvqError, match="outside the pool"):
        ops.stream_stage_window_slots(state, [0, 2], 12, src, 5, 16, 12, cap)
    with pytest.raises(MvqError, match="does not fit"):
        ops.stream_stage_window(state, 12, src, 5, 16, 12, cap, tail_off=4)
    torch.cuda.synchronize()
    assert bool(torch.isnan(win).all()) and bool((state == 3.0).all())                             # nothing ran


# ---------------------------------------------------------------------------------------------------- 2. the stack call
def _latent(dev, B, T):
    """Seeded latents and decoder_fwd of the whole of them -- once per (B, T)."""
    if ("z", B, T) not in _REF:
        z = (0.5 * torch.randn(B, 1024, T, generator=torch.Generator(device="cpu").manual_seed(100 * B + T))).to(dev)
        _REF[("z", B, T)] = (z, _net(dev).T_DEC.stack().decoder_fwd(z))
    return _REF[("z", B, T)]


def _stack_pieces(st, state, z, pieces, slots=None):
    """decoder_stream_fwd over ``pieces`` (tokens per push) and a finish with what remains -> the outputs."""
    out, at = [], 0
    for n in pieces:
        out.append(st.decoder_stream_fwd(state, z[..., at:at + n].contiguous(), at, False, slots=slots))
        at += n
    out.append(st.decoder_stream_fwd(state, z[..., at:].contiguous(), at, True, slots=slots))
    return out


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("T", [11, 16, 37, 75])
def test_stack_stream_fwd_equals_whole_item_decode(T, B, dev):
    st = _net(dev).T_DEC.stack()
    z, want = _latent(dev, B, T)
    assert want.shape == (B, 1, 320 * T - 8)
    state = st.decoder_stream_state(B, device=dev)
    assert state.shape == (B, st.decoder_stream_state_floats()) and state.shape[1] == sum(
        c * t for c, t in zip((1024, 1536, 768, 384, 192, 96), stream.DEC_STAGE_TAILS))
    state.fill_(NAN)                                                         # a new session reads none of it
    out = _stack_pieces(st, state, z, [16] * (T // 16))
    assert [y.shape[-1] for y in out] == [e1 - e0 for _, _, e0, e1 in stream.schedule(T)]
    assert torch.equal(torch.cat(out, dim=-1), want)


@pytest.mark.parametrize("B,T", [(32, 75), (35, 11)])
def test_stack_stream_fwd_on_packed_latent_rows(B, T, dev):
    """From 32 sessions on the head runs on packed latent-rate rows, as decoder_fwd's does: full rows (32 = 4 x 8) and a last row
    that is not full (35), dense and through a slot list."""
    st = _net(dev).T_DEC.stack()
    z, want = _latent(dev, B, T)
    state = st.decoder_stream_state(B, device=dev).fill_(NAN)
    out = _stack_pieces(st, state, z, [16] * (T // 16))
    assert torch.equal(torch.cat(out, dim=-1), want)
    slots = [(7 * i) % 37 for i in range(B)]                                # a permutation of 0..36 taken B at a time
    assert len(set(slots)) == B
    pool = st.decoder_stream_state(37, device=dev).fill_(NAN)
    got = _stack_pieces(st, pool, z, [16] * (T // 16), slots=slots)
    assert all(torch.equal(a, b) for a, b in zip(out, got))


def test_stack_stream_fwd_any_piece_sizes_and_slots(dev):
    """Pieces that are no chunks (the plan is general), and the same sessions through a slot list into a larger state."""
    st = _net(dev).T_DEC.stack()
    z, want = _latent(dev, 3, 37)
    pieces = [5, 16, 1, 9]
    state = st.decoder_stream_state(3, device=dev).fill_(NAN)
    out = _stack_pieces(st, state, z, pieces)
    assert [y.shape[-1] for y in out] == [0, 3520, 320, 2880, 5112]          # 320 * (N - 10) from N = 5, 21, 22, 31, then the rest
    assert torch.equal(torch.cat(out, dim=-1), want)
    pool = st.decoder_stream_state(5, device=dev).fill_(NAN)
    got = _stack_pieces(st, pool, z, pieces, slots=[4, 0, 2])
    assert all(torch.equal(a, b) for a, b in zip(out, got))
    assert torch.equal(_bits(pool[[4, 0, 2]]), _bits(state)) and bool(torch.isnan(pool[[1, 3]]).all())


# ------------------------------------------------------------------------------------------------- 3. the session object
@pytest.mark.parametrize("conceal", ["predict", "zero"])
@pytest.mark.parametrize("T", [75, 37])
def test_stateful_receiver_equals_window_mode_call_by_call(T, conceal, dev):
    net = _net(dev)
    infos, rx, aud, codes, _ = _case(dev, T)
    for out_rate in (24000, 3000):
        win = _run_session(net.stream_receiver(512, 8, batch=2, conceal=conceal, out_rate=out_rate), rx, codes, T, extra_late=True)
        rxs = net.stream_receiver(512, 8, batch=2, conceal=conceal, out_rate=out_rate, decoder="stateful")
        assert rxs.hist is None and rxs.dec_state.shape[0] == 2
        got = _run_session(rxs, rx, codes, T, extra_late=True)
        assert len(got) == len(win) == T // 16 + 1
        for i, (a, b) in enumerate(zip(got, win)):
            assert a.shape == b.shape and torch.equal(a, b), (out_rate, i)
        if out_rate == 24000:
            assert torch.equal(torch.cat(got, dim=-1), _whole(dev, T, conceal))
    assert rxs.finished and rxs.tokens == T


def test_stateful_receiver_with_audio_packets_and_fec(dev):
    """audio=(K_a, na) with fec= and audio_fec=: what acts before the latents is untouched by the decoder mode."""
    import fec_channel as fc
    import sender_oracle as sn
    import test_gpu_fec as tf
    net = tf._net(dev)
    B, L = 2, 320 * 59                                                       # three whole chunks and a tail of 11 tokens
    a, t = tf._signals(dev, B, L)
    tx = net.stream_sender(batch=B, rate=tf.RATE, audio="packets", audio_rate=tf.ARATE, fec=tf.FEC, audio_fec=tf.AFEC)
    out, (info, ainfo) = tf._run_sender(tx, a, t, sn.split_pushes(L, 16, seed=3), 2)
    pk, apk, par, apar = ([tf._cat(out, k, b) for b in range(B)] for k in range(4))
    rx_pk, rx_par, _, _ = tf._lossy(pk, par, info, tf.FEC, 1)
    rx_apk, rx_apar, _, _ = tf._lossy(apk, apar, ainfo, tf.AFEC, 2)
    want = net.decompress_packets_av([info] * B, rx_pk, [ainfo] * B, rx_apk, fec=tf.FEC, fec_packets=rx_par, audio_fec=tf.AFEC,
                                     audio_fec_packets=rx_apar)[0]
    runs = {}
    for mode in ("window", "stateful"):
        rx = net.stream_receiver(512, 8, batch=B, audio=(1024, 32), fec=tf.FEC, audio_fec=tf.AFEC, decoder=mode)
        ys = []
        for c in range(info.T // 16):
            pick = lambda lists, n=8: [[p for p in lists[b] if n * c <= fc.seq_of(p) < n * c + n] for b in range(B)]
            ys.append(rx.push(pick(rx_pk), audio_packets=pick(rx_apk), fec_packets=pick(rx_par, 2), audio_fec_packets=pick(rx_apar, 2)))
        tail = lambda lists, n=8: [[p for p in lists[b] if fc.seq_of(p) >= n * (info.T // 16)] for b in range(B)]
        ys.append(rx.finish(tail(rx_pk), tail(rx_apk), tokens=info.T % 16, fec_packets=tail(rx_par, 2), audio_fec_packets=tail(rx_apar, 2)))
        runs[mode] = ys
    assert all(torch.equal(x, y) for x, y in zip(runs["stateful"], runs["window"]))
    assert torch.equal(torch.cat(runs["stateful"], dim=-1), want)


def test_stateful_receiver_with_audio_conceal_hold(dev):
    import test_gpu_audio_conceal as tac
    import test_gpu_av as tav
    net = tav._net(dev)
    B, T = 2, 37
    a, t = tav._signals(dev, B, 320 * T)
    infos, pk, ainfos, apk = net.compress_packets_av(a, t)
    info, ainfo = infos[0], ainfos[0]
    rx_pk = [tav._channel(pk[b], info, 10 * b + 1)[0] for b in range(B)]
    rx_apk = tac._audio_drops(apk, T)
    want = net.decompress_packets_av([info] * B, rx_pk, [ainfo] * B, rx_apk, audio_conceal="hold")[0]
    runs = {}
    for mode in ("window", "stateful"):
        rx = net.stream_receiver(512, 8, batch=B, audio=(1024, 32), audio_conceal="hold", decoder=mode)
        ys = []
        for c in range(T // 16):
            pick = lambda lists: [[p for p in lists[b] if 8 * c <= _seq(p) < 8 * c + 8] for b in range(B)]
            ys.append(rx.push(pick(rx_pk), audio_packets=pick(rx_apk)))
        tail = lambda lists: [[p for p in lists[b] if _seq(p) >= 8 * (T // 16)] for b in range(B)]
        ys.append(rx.finish(tail(rx_pk), tail(rx_apk), tokens=T % 16))
        runs[mode] = ys
    assert all(torch.equal(x, y) for x, y in zip(runs["stateful"], runs["window"]))
    assert torch.equal(torch.cat(runs["stateful"], dim=-1), want)


# --------------------------------------------------------------------------------------------------------------- 4. graph
def test_stateful_receiver_graph_replays_the_steady_step(dev):
    """Six full chunks: the captured step (from the third push on) is replayed three times after its capture, under a different
    loss pattern each time, and equals the eager stateful session call by call."""
    net = _net(dev)
    T, B = 96, 1
    r = np.random.default_rng(96)
    info = StreamInfo(512, 8, T, 2)
    pk = packets.frame(packets.pack_bodies(r.integers(0, 512, size=(8, T)), info), info)
    codes = torch.from_numpy(r.integers(0, 1024, size=(B, 32, T)))
    keep = []
    for c in range(6):
        mine = pk[8 * c:8 * c + 8]
        mine = {1: mine[::2], 2: [packets.thin(p, 1 + j % 7, info) for j, p in enumerate(mine)], 3: mine[:6], 4: [],
                5: [p for p in mine if r.random() < 0.6][::-1]}.get(c, mine)
        keep += mine
    eager = _run_session(net.stream_receiver(512, 8, batch=B, decoder="stateful"), [keep], codes, T)
    rxg = net.stream_receiver(512, 8, batch=B, graph=True, decoder="stateful")
    graphed = _run_session(rxg, [keep], codes, T)
    assert rxg._g is not None and isinstance(rxg._g[0], torch.cuda.CUDAGraph)
    assert len(eager) == len(graphed) == 7 and all(y.shape == (1, 1, 5120) for y in eager[2:6])
    assert len({y.cpu().numpy().tobytes() for y in eager[2:6]}) == 4        # four different outputs of the one graph
    for i, (a, b) in enumerate(zip(eager, graphed)):
        assert torch.equal(a, b), i
    want = net.decompress_packets([info], [keep], [bitstream.pack_indices(codes[0].numpy(), 1024)])[0]
    assert torch.equal(torch.cat(graphed, dim=-1), want)


# ---------------------------------------------------------------------------------------------------------------- 5. pool
def test_stateful_pool_equals_solo_sessions_and_the_window_pool(dev):
    from test_gpu_stream_pool import ITEMS, OPENS, _drive
    net = _net(dev)
    pool = net.stream_receiver_pool(512, 8, slots=4, decoder="stateful")
    assert pool.hist is None and pool.dec_state.shape[0] == 4
    pool.dec_state.fill_(NAN)                                               # open() clears none of it: a new session reads no tail
    outs, _, slot = _drive(pool, dev, ITEMS, OPENS, straggler=0)
    assert pool.active == () and pool.free == 4
    assert slot[4] in (slot[1], slot[2], slot[3])                           # the fifth session runs on a freed slot's stale state
    wouts, _, _ = _drive(net.stream_receiver_pool(512, 8, slots=4), dev, ITEMS, OPENS, straggler=0)
    for i, (T, b) in enumerate(ITEMS):
        _, rx, _, codes, _ = _case(dev, T)
        solo = _run_session(net.stream_receiver(512, 8, batch=1, decoder="stateful"), [rx[b]], codes[b:b + 1], T, extra_late=(i == 0))
        assert len(outs[i]) == len(solo) == len(wouts[i])
        for k, (a, s, w) in enumerate(zip(outs[i], solo, wouts[i])):
            assert a.shape == s.shape and not bool(torch.isnan(a).any()) and torch.equal(a, s) and torch.equal(a, w), (T, b, k)


# ----------------------------------------------------------------------------------------------------------- 6. refusals
def test_stateful_refusals_come_before_any_launch(dev):
    from multimodal_vqvae_compression_audio_tactile_amd import _lib, ops
    net = _net(dev)
    st = net.T_DEC.stack()
    L = _lib.lib()
    B, n, before = 2, 16, 32
    z = torch.ones(B, 1024, n, device=dev)
    state = torch.full((B, st.decoder_stream_state_floats()), 3.0, device=dev)
    y = torch.full((B, 1, 5120), NAN, device=dev)
    need = int(L.mvq_decoder_stream_workspace_bytes(st.handle, B, before, n, 0))
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    call = lambda y_len, nbytes: L.mvq_decoder_stream_fwd_f32(st.handle, state.data_ptr(), None, B, B, z.data_ptr(), n, before, 0, y.data_ptr(),
                                                               y_len, ws.data_ptr(), nbytes, _stream())
    assert call(5120, need // 2) == -1 and b"workspace too small" in L.mvq_last_error()
    assert call(5119, need) == -1 and b"y_len = 5119" in L.mvq_last_error() and b"5120" in L.mvq_last_error()
    assert L.mvq_decoder_stream_fwd_f32(st.handle, state.data_ptr(), None, 3, B, z.data_ptr(), n, before, 0, y.data_ptr(), 5120, ws.data_ptr(),
                                        need, _stream()) == -1                                      # more sessions than state rows
    with ops.arith("f16x3"):
        with pytest.raises(ValueError, match="f16x3"):
            st.decoder_stream_fwd(state, z, before)
        with pytest.raises(ValueError, match="f16x3"):
            net.stream_receiver(512, 8, decoder="stateful")
    with pytest.raises(ValueError, match="state"):
        st.decoder_stream_fwd(state[:, :-1], z, before)
    with pytest.raises(ValueError, match="decoder must be"):
        net.stream_receiver(512, 8, decoder="bogus")
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all()) and bool((state == 3.0).all())                               # nothing ran
