"""-m gpu: the receiver pool on the device -- the three slot kernels against torch indexing and the
per-session StreamResample, StreamReceiverPool end to end against decompress_packets of each item alone (staggered starts,
different lengths, a slot reused after a finish), one item alone against the same item among others, and the refusals.
Every comparison is an equality.  The model, the items and their loss patterns are those of tests/test_gpu_stream.py."""
import pytest
import torch

from multimodal_vqvae_compression_audio_tactile_amd import stream
from test_gpu_stream import GUARD, WINDOW_SHAPES, _case, _net, _seq, _stream

pytestmark = pytest.mark.gpu

_ALONE = {}
S_POOL = 5
LISTS = [[3], [4, 0, 2]]


def _nan(n, dev):
    return torch.full((n,), float("nan"), device=dev)


# ------------------------------------------------------------------------------------------------------- 1. slot kernels
@pytest.mark.parametrize("C", [96, 1024])
def test_stream_window_slots_equals_indexed_cat_and_slicing(C, dev):
    from multimodal_vqvae_compression_audio_tactile_amd import _lib, ops
    cap, S = 20, S_POOL
    g = torch.Generator(device="cpu").manual_seed(C)
    for slots in LISTS:
        G = len(slots)
        sd = torch.tensor(slots, dtype=torch.int32, device=dev)
        for h_in, n, h_out in WINDOW_SHAPES:
            hist0 = torch.randn(S, C, cap, generator=g).to(dev)
            z = torch.randn(G, C, n, generator=g).to(dev)
            want_win = torch.cat([hist0[slots][..., :h_in], z], dim=2)
            want_hist = hist0.clone()
            want_hist[slots, :, :h_out] = want_win[..., h_in + n - h_out:]       # unlisted slots: bit-identical to before
            hist = hist0.clone()
            win = ops.stream_window_slots(hist, slots, h_in, z, h_out)
            assert win.shape == (G, C, h_in + n) and win.is_contiguous()
            assert torch.equal(win, want_win) and torch.equal(hist, want_hist), (slots, h_in, n, h_out)
            hist = hist0.clone()                                                  # the list uploaded by the caller
            assert torch.equal(ops.stream_window_slots(hist, slots, h_in, z, h_out, slots_dev=sd), want_win) and torch.equal(hist, want_hist)
            # the C entry point into NaN-filled outputs with a guard band behind them
            W = h_in + n
            out = _nan(G * C * W + GUARD, dev)
            hbuf = torch.cat([hist0.reshape(-1), _nan(GUARD, dev)])
            rc = _lib.lib().mvq_stream_window_slots_f32(hbuf.data_ptr(), sd.data_ptr(), G, S, h_in, z.data_ptr(), n, out.data_ptr(), h_out,
                                                        cap, C, _stream())
            assert rc == 0
            assert torch.equal(out[:G * C * W].view(G, C, W), want_win) and bool(torch.isnan(out[G * C * W:]).all())
            assert torch.equal(hbuf[:S * C * cap].view(S, C, cap), want_hist) and bool(torch.isnan(hbuf[S * C * cap:]).all())
    # the kernel's own range check (the wrapper never lets such a list through): zeros are read, nothing is stored
    hist0 = torch.randn(S, C, cap, generator=g).to(dev)
    z = torch.randn(2, C, 16, generator=g).to(dev)
    hbuf = torch.cat([hist0.reshape(-1), _nan(GUARD, dev)])
    out = _nan(2 * C * 36 + GUARD, dev)
    sd = torch.tensor([S, -1], dtype=torch.int32, device=dev)
    assert _lib.lib().mvq_stream_window_slots_f32(hbuf.data_ptr(), sd.data_ptr(), 2, S, 20, z.data_ptr(), 16, out.data_ptr(), 20, cap, C,
                                                  _stream()) == 0
    assert torch.equal(out[:2 * C * 36].view(2, C, 36), torch.cat([torch.zeros(2, C, 20, device=dev), z], dim=2))
    assert bool(torch.isnan(out[2 * C * 36:]).all())
    assert torch.equal(hbuf[:S * C * cap].view(S, C, cap), hist0) and bool(torch.isnan(hbuf[S * C * cap:]).all())


@pytest.mark.parametrize("C", [96, 1024])
def test_stream_rows_gathers_and_scatters(C, dev):
    from multimodal_vqvae_compression_audio_tactile_amd import _lib, ops
    S = S_POOL
    g = torch.Generator(device="cpu").manual_seed(7 + C)
    for slots in LISTS:
        G = len(slots)
        sd = torch.tensor(slots, dtype=torch.int32, device=dev)
        pool0 = torch.randn(S, C, generator=g).to(dev)
        rows = torch.randn(G, C, generator=g).to(dev)
        pool = pool0.clone()
        got = ops.stream_rows(pool, slots)
        assert got.shape == (G, C) and torch.equal(got, pool0[slots]) and torch.equal(pool, pool0)
        want = pool0.clone()
        want[slots] = rows
        assert ops.stream_rows(pool, slots, rows=rows, slots_dev=sd) is pool and torch.equal(pool, want)
        # the C entry point, both directions, into NaN-filled / guarded buffers
        out = _nan(G * C + GUARD, dev)
        pbuf = torch.cat([pool0.reshape(-1), _nan(GUARD, dev)])
        assert _lib.lib().mvq_stream_rows_f32(pbuf.data_ptr(), sd.data_ptr(), G, S, out.data_ptr(), C, 0, _stream()) == 0
        assert torch.equal(out[:G * C].view(G, C), pool0[slots]) and bool(torch.isnan(out[G * C:]).all())
        assert torch.equal(pbuf[:S * C].view(S, C), pool0)
        assert _lib.lib().mvq_stream_rows_f32(pbuf.data_ptr(), sd.data_ptr(), G, S, rows.data_ptr(), C, 1, _stream()) == 0
        assert torch.equal(pbuf[:S * C].view(S, C), want) and bool(torch.isnan(pbuf[S * C:]).all())
    # the kernel's own range check: zeros gathered, nothing scattered
    sd = torch.tensor([-1, S], dtype=torch.int32, device=dev)
    pool0 = torch.randn(S, C, generator=g).to(dev)
    pbuf = torch.cat([pool0.reshape(-1), _nan(GUARD, dev)])
    out = _nan(2 * C + GUARD, dev)
    assert _lib.lib().mvq_stream_rows_f32(pbuf.data_ptr(), sd.data_ptr(), 2, S, out.data_ptr(), C, 0, _stream()) == 0
    assert not out[:2 * C].any() and bool(torch.isnan(out[2 * C:]).all())
    ones = torch.ones(2, C, device=dev)
    assert _lib.lib().mvq_stream_rows_f32(pbuf.data_ptr(), sd.data_ptr(), 2, S, ones.data_ptr(), C, 1, _stream()) == 0
    assert torch.equal(pbuf[:S * C].view(S, C), pool0) and bool(torch.isnan(pbuf[S * C:]).all())


def test_resample_stream_slots_equals_the_session_resampler(dev):
    """Slots 4 and 0 take the pieces [1920, 5120, 1592] as one group (consumed 0, 1920, 7040), slot 1 takes [3512] at once in a
    group of its own (its launch class differs: final at consumed 0); against StreamResample(batch=1) per session."""
    from multimodal_vqvae_compression_audio_tactile_amd import StreamResample, ops
    from multimodal_vqvae_compression_audio_tactile_amd.resample import sinc_resample_kernel
    kern, width, orig, new = sinc_resample_kernel(24000, 3000)
    kern = kern.to(dev)
    state = ops.resample_stream_state(orig, width, S_POOL, dev)
    state[2].fill_(5.0), state[3].fill_(-3.0)                                   # slots of other sessions
    g = torch.Generator().manual_seed(11)
    pieces, L = [1920, 5120, 1592], 8632
    x = torch.randn(3, L, generator=g).to(dev)                                  # sessions in slots 4, 0 and 1
    want = []
    for i in range(2):
        rs = StreamResample(24000, 3000, 1, device=dev)
        pos, outs = 0, []
        for j, n in enumerate(pieces):
            outs.append(rs.finish(x[i:i + 1, pos:pos + n]) if j == 2 else rs.push(x[i:i + 1, pos:pos + n]))
            pos += n
        want.append(outs)
    rs = StreamResample(24000, 3000, 1, device=dev)
    want_b = rs.finish(x[2:3, :3512])
    pos, lens = 0, [233, 640, 206]
    for j, n in enumerate(pieces):
        y = ops.resample_stream_slots(x[:2, pos:pos + n], kern, state, [4, 0], pos, orig, new, width, final=j == 2)
        assert y.shape == (2, lens[j])
        assert torch.equal(y[0:1], want[0][j]) and torch.equal(y[1:2], want[1][j]), j
        if j == 0:                                                              # the other group, between the first one's steps
            yb = ops.resample_stream_slots(x[2:3, :3512], kern, state, [1], 0, orig, new, width, final=True)
            assert yb.shape == (1, 439) and torch.equal(yb, want_b)
        pos += n
        if j < 2:
            assert torch.equal(state[[4, 0]], x[:2, pos - 105:pos])             # the last 105 samples, oldest first
    assert bool((state[2] == 5.0).all()) and bool((state[3] == -3.0).all())     # unlisted slots: untouched
    # a launch class is a property of the group: any consumed >= 105 gives the steady launch
    st2 = ops.resample_stream_state(orig, width, 2, dev)
    st2[1] = x[0, 1920 - 105:1920]
    y = ops.resample_stream_slots(x[:1, 1920:7040], kern, st2, [1], 7040 + 5120 * 9, orig, new, width)
    assert torch.equal(y, want[0][1]) and not st2[0].any()


# ------------------------------------------------------------------------------------------------------- 2. end to end
ITEMS = [(75, 0), (37, 1), (16, 0), (11, 1), (40, 0)]            # (tokens, which item of test_gpu_stream._case(T))
OPENS = [0, 0, 1, 2, 3]                                           # the tick each session opens at


def _alone(dev, T, b, conceal):
    """decompress_packets of that item alone -- once per (T, item, conceal)."""
    if (T, b, conceal) not in _ALONE:
        infos, rx, aud, _, _ = _case(dev, T)
        _ALONE[(T, b, conceal)] = _net(dev).decompress_packets([infos[b]], [rx[b]], [aud[b]], conceal=conceal)[0]
    return _ALONE[(T, b, conceal)]


def _drive(pool, dev, items, opens, straggler=None):
    """Run the sessions of ``items`` through ``pool``, session i opening at tick opens[i]; each tick pushes the next full chunk
    of every open session and finishes the ones that have none left.  ``straggler``: the item that is handed two packets of its
    chunk 0 again with its chunk 2.  -> (outputs per item, late count after each push per item, the slot each session held)."""
    per = 16 // pool.packet_tok
    data = [(_case(dev, T)[1][b], _case(dev, T)[3][b], T) for T, b in items]
    sids, nxt, done, slot = {}, {}, set(), {}
    outs, lates = {i: [] for i in range(len(items))}, {i: [] for i in range(len(items))}
    tick = 0
    while len(done) < len(items):
        for i, t0 in enumerate(opens):
            if t0 == tick:
                sids[i], nxt[i] = pool.open(), 0
                slot[i] = pool._sess[sids[i]][0]
        pushes, finishes = {}, {}
        for i, sid in sids.items():
            if i in done:
                continue
            rx, codes, T = data[i]
            c = nxt[i]
            if 16 * (c + 1) <= T:
                mine = [p for p in rx if c * per <= _seq(p) < (c + 1) * per]
                if i == straggler and c == 2:
                    mine = mine + [p for p in rx if _seq(p) < per][:2]
                pushes[sid] = (mine, codes[:, 16 * c:16 * c + 16] if i % 2 else codes[None, :, 16 * c:16 * c + 16])
            else:
                finishes[sid] = ([p for p in rx if _seq(p) >= c * per], codes[:, 16 * c:]) if T % 16 else None
        out = pool.step(pushes, finishes)
        assert sorted(out) == sorted(list(pushes) + list(finishes))
        for i, sid in sids.items():
            if sid in out:
                outs[i].append(out[sid])
            if sid in pushes:
                nxt[i] += 1
                assert pool.tokens(sid) == 16 * nxt[i]
                lates[i].append(pool.late(sid))
            elif sid in finishes:
                done.add(i)
        tick += 1
    return outs, lates, slot


@pytest.mark.parametrize("conceal,out_rate", [("predict", 24000), ("zero", 24000), ("predict", 3000)])
def test_pool_equals_decompress_packets_per_session(conceal, out_rate, dev):
    from multimodal_vqvae_compression_audio_tactile_amd import MvqError, Resample
    net = _net(dev)
    pool = net.stream_receiver_pool(512, 8, slots=4, conceal=conceal, out_rate=out_rate)
    outs, lates, slot = _drive(pool, dev, ITEMS, OPENS, straggler=0)
    assert pool.active == () and pool.free == 4
    assert slot[4] in (slot[1], slot[2], slot[3]) and len({slot[i] for i in range(4)}) == 4      # the fifth session reuses a freed slot
    for i, (T, b) in enumerate(ITEMS):
        want = _alone(dev, T, b, conceal)
        assert want.shape == (1, 1, 320 * T - 8)
        assert all(y.shape[:2] == (1, 1) for y in outs[i])
        if out_rate == 24000:
            assert [y.shape[-1] for y in outs[i]] == [e1 - e0 for _, _, e0, e1 in stream.schedule(T)]
        else:
            want = Resample(24000, 3000).to(dev)(want)
            assert want.shape == (1, 1, 40 * T - 1)
        got = torch.cat(outs[i], dim=-1)
        assert got.shape == want.shape and torch.equal(got, want), (T, b)
    # the straggler's packets were counted for its session alone, from the tick they came with
    rx0 = _case(dev, 75)[1][0]
    n_late = min(2, len([p for p in rx0 if _seq(p) < 8]))
    assert lates[0] == [0, 0, n_late, n_late]
    assert all(v == 0 for i in range(1, 5) for v in lates[i])
    with pytest.raises(MvqError, match="no open session"):
        pool.step({0: ([], torch.zeros(32, 16, dtype=torch.int64))})


def test_steady_group_mixes_sessions_of_different_age(dev):
    """Two sessions one tick apart: from the second's third chunk on they share the steady group (32 and 48 tokens before)."""
    net = _net(dev)
    pool = net.stream_receiver_pool(512, 8, slots=2)
    outs, _, _ = _drive(pool, dev, [(75, 0), (75, 1)], [0, 1])
    for i in range(2):
        assert torch.equal(torch.cat(outs[i], dim=-1), _alone(dev, 75, i, "predict"))


# ----------------------------------------------------------------------------------------------- 3. alone equals among
def test_an_item_alone_equals_the_item_among_others(dev):
    net = _net(dev)
    among, _, _ = _drive(net.stream_receiver_pool(512, 8, slots=4), dev, ITEMS, OPENS)
    for i in (1, 4):
        alone, _, _ = _drive(net.stream_receiver_pool(512, 8, slots=4), dev, [ITEMS[i]], [0])
        assert len(alone[0]) == len(among[i])
        for a, b in zip(alone[0], among[i]):
            assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------------ 4. refusals
def test_pool_refusals_on_the_device(dev):
    from multimodal_vqvae_compression_audio_tactile_amd import MvqError
    net = _net(dev)
    with pytest.raises(ValueError, match="plc"):
        net.stream_receiver_pool(512, 8, conceal="plc")
    with pytest.raises(ValueError, match="K = 128"):
        net.stream_receiver_pool(128, 8)
    pool = net.stream_receiver_pool(512, 8, slots=2)
    a, b = pool.open(), pool.open()
    with pytest.raises(MvqError, match="all 2 slots"):
        pool.open()
    codes = torch.zeros(32, 16, dtype=torch.int64)
    with pytest.raises(MvqError, match="no open session 7"):
        pool.step({a: ([], codes), 7: ([], codes)})
    with pytest.raises(ValueError, match="17 audio tokens"):
        pool.step({a: ([], codes), b: ([], torch.zeros(32, 17, dtype=torch.int64))})
    with pytest.raises(ValueError, match="audio_codes must be int"):
        pool.step({a: ([], codes), b: ([], torch.zeros(2, 32, 16, dtype=torch.int64))})
    with pytest.raises(ValueError, match="30 audio code rows"):
        pool.step({a: ([], codes)}, {b: ([], torch.zeros(30, 5, dtype=torch.int64))})
    with pytest.raises(ValueError, match="both"):
        pool.step({a: ([], codes)}, {a: None})
    torch.cuda.synchronize()
    assert (pool.tokens(a), pool.tokens(b)) == (0, 0) and not pool.carry.any() and not pool.hist.any()      # nothing ran
    out = pool.step({a: ([], codes.to(dev))}, {b: ([], codes[:, :5])})
    assert out[a].shape == (1, 1, 1920) and out[b].shape == (1, 1, 320 * 5 - 8)
    assert pool.active == (a,) and pool.free == 1 and pool.tokens(a) == 16
    with pytest.raises(MvqError, match="no open session"):                     # push after finish
        pool.step({b: ([], codes)})
    with pytest.raises(MvqError, match="no open session"):
        pool.step({}, {b: None})
    tail = pool.step({}, {a: None})[a]
    assert tail.shape == (1, 1, 5112 - 1920) and pool.active == () and pool.free == 2
