"""-m gpu: the sender pool on the device -- the slot instantiation of the sample-state kernel against
torch.cat / slicing and against the dense call, the kernel's own descriptor check, StreamSenderPool end to end against
compress_packets of each item alone (staggered starts, ragged pushes, different lengths, a slot reused after a finish), a pool
session against a solo StreamSender step by step, the sender pool feeding the receiver pool over a lossy channel, and the
refusals.  Every comparison is an equality.  The model, the items and the helpers are those of tests/test_gpu_sender.py."""
import pytest
import torch

import sender_oracle as sn
from multimodal_vqvae_compression_audio_tactile_amd import bitstream, stream
from multimodal_vqvae_compression_audio_tactile_amd.packets import StreamInfo
from test_gpu_sender import CAP, GUARD, LENGTHS, _case, _channel, _check_session, _net, _seq, _stream

pytestmark = pytest.mark.gpu

S_POOL = 5
LISTS = [[3], [4, 0, 2]]
# w -> the (fill, n, drop) of the members of a group: one window length per launch, everything else per session
GROUPS = [
    (10240, [(5120, 5120, 5120), (7680, 5120, 5120), (9920, 320, 5120)]),     # the steady emit from three different fills
    (0, [(2560, 1600, 0), (15040, 320, 0), (0, 320, 0)]),                     # the append group; one append fills the buffer
    (100, [(12000, 3000, 7), (4097, 1, 1)]),                                  # shifts by 7 and by 1: nothing aligned
    (7543, [(5120, 2423, 7543), (7000, 543, 7543)]),                          # finishers: everything out, nothing kept
    (20480, [(15360, 5120, 5120)]),                                           # a full buffer moved on and full again
]


def _nan(n, dev):
    return torch.full((n,), float("nan"), device=dev)


def _reference(buf0, slots, members, xs, w):
    """torch.cat / slicing per session and modality -> (win [2, G, w], the pool afterwards)."""
    G = len(slots)
    want_win = torch.empty(2, G, w, device=buf0.device)
    want_buf = buf0.clone()
    for g, (slot, (fill, n, drop)) in enumerate(zip(slots, members)):
        for m in range(2):
            v = torch.cat([buf0[slot, m, :fill], xs[g][m]])
            want_win[m, g] = v[:w]
            want_buf[slot, m, :fill + n - drop] = v[drop:]
    return want_win, want_buf


# ------------------------------------------------------------------------------------------------------ 1. the slot kernel
def test_stream_samples_slots_equals_cat_and_slicing(dev):
    from multimodal_vqvae_compression_audio_tactile_amd import _lib, ops
    S = S_POOL
    gen = torch.Generator(device="cpu").manual_seed(17)
    for slots in LISTS:
        G = len(slots)
        for w, params in GROUPS:
            runs = [[p] for p in params] if G == 1 else [[params[i % len(params)] for i in range(G)]]
            for members in runs:
                buf0 = torch.randn(S, 2, CAP, generator=gen).to(dev)
                xs = [torch.randn(2, n, generator=gen).to(dev) for _, n, _ in members]
                x = torch.cat([v.reshape(-1) for v in xs])                            # per session: audio, then tactile
                sessions = [(slot, *p) for slot, p in zip(slots, members)]
                want_win, want_buf = _reference(buf0, slots, members, xs, w)
                buf = buf0.clone()
                win = ops.stream_samples_slots(buf, sessions, x, w)
                assert win.shape == (2, G, w) and win.is_contiguous()
                assert torch.equal(win, want_win) and torch.equal(buf, want_buf), (slots, w, members)   # unlisted slots: bit-identical
                rows, x_total = ops.stream_samples_desc(sessions, w, CAP)
                assert x_total == x.numel()
                dd = torch.tensor(rows, dtype=torch.int32, device=dev)                # the table uploaded by the caller
                buf = buf0.clone()
                assert torch.equal(ops.stream_samples_slots(buf, sessions, x, w, desc_dev=dd), want_win) and torch.equal(buf, want_buf)
                # the C entry point into NaN-filled outputs with a guard band behind them
                out = _nan(2 * G * w + GUARD, dev)
                bbuf = torch.cat([buf0.reshape(-1), _nan(GUARD, dev)])
                rc = _lib.lib().mvq_stream_samples_slots_f32(bbuf.data_ptr(), dd.data_ptr(), G, S, x.data_ptr(), x_total, out.data_ptr(), w,
                                                             CAP, _stream())
                assert rc == 0
                assert torch.equal(out[:2 * G * w].view(2, G, w), want_win) and bool(torch.isnan(out[2 * G * w:]).all()), (slots, w)
                assert torch.equal(bbuf[:S * 2 * CAP].view(S, 2, CAP), want_buf) and bool(torch.isnan(bbuf[S * 2 * CAP:]).all())


def test_stream_samples_slots_identity_equals_the_dense_call(dev):
    from multimodal_vqvae_compression_audio_tactile_amd import ops
    S = S_POOL
    gen = torch.Generator(device="cpu").manual_seed(23)
    for fill, n, w, drop in ((5120, 5120, 10240, 5120), (2560, 1600, 0, 0), (12000, 3000, 100, 7), (15360, 5120, 20480, 5120)):
        pool0 = torch.randn(S, 2, CAP, generator=gen).to(dev)
        xs = torch.randn(S, 2, n, generator=gen).to(dev)
        dense = pool0.permute(1, 0, 2).reshape(2 * S, CAP).contiguous()               # audio rows, then tactile rows
        win_d = ops.stream_samples(dense, fill, xs.permute(1, 0, 2).reshape(2 * S, n).contiguous(), w, drop)
        pool = pool0.clone()
        win_p = ops.stream_samples_slots(pool, [(s, fill, n, drop) for s in range(S)], xs.reshape(-1), w)
        assert torch.equal(win_p.view(2 * S, w), win_d) and torch.equal(pool.permute(1, 0, 2).reshape(2 * S, CAP), dense)


def test_stream_samples_slots_host_refusals_on_the_device(dev):
    from multimodal_vqvae_compression_audio_tactile_amd import MvqError, ops
    buf = torch.full((4, 2, CAP), 3.0, device=dev)
    x = torch.ones(2 * 320 + 2 * 640, device=dev)
    good = [(3, 5120, 320, 0), (0, 0, 640, 0)]
    dd = torch.tensor(ops.stream_samples_desc(good, 0, CAP)[0], dtype=torch.int32, device=dev)
    bad = [
        ([(3, 5120, 320, 0), (3, 0, 640, 0)], x, 0, None), ([(4, 5120, 320, 0), (0, 0, 640, 0)], x, 0, None),
        ([(3, 15360, 320, 319), (0, 0, 640, 0)], x, 0, None), ([(3, 5120, 320, 5441), (0, 0, 640, 0)], x, 0, None),
        (good, x, 641, None), (good, x[:-1], 0, None), (good, x.cpu(), 0, None), (good, x.double(), 0, None),
        (good, x, 0, dd.cpu()), (good, x, 0, dd.long()), (good, x, 0, dd[:1]), (good, x, 0, dd.reshape(-1)),
    ]
    for sessions, xs, w, desc in bad:
        with pytest.raises(MvqError):
            ops.stream_samples_slots(buf, sessions, xs, w, desc_dev=desc)
    with pytest.raises(MvqError):
        ops.stream_samples_slots(buf[:, :, :10240], good, x, 0)                       # not contiguous: the pitch is the capacity
    torch.cuda.synchronize()
    assert bool((buf == 3.0).all())                                                   # nothing ran
    assert ops.stream_samples_slots(buf, good, x, 0, desc_dev=dd).shape == (2, 2, 0)
    assert bool((buf[3, :, 5120:5440] == 1.0).all()) and bool((buf[0, :, :640] == 1.0).all()) and bool((buf[1:3] == 3.0).all())


# ------------------------------------------------------------------------------------------- 2. the kernel's own check
def test_stream_samples_slots_kernel_checks_its_descriptors(dev):
    """Through the C entry point (the wrapper never lets such a table through).  The pool and x_new are views in the MIDDLE of
    larger allocations, a slot block of margin on each side: a missing check shows as a changed margin, not as an access out
    of bounds."""
    from multimodal_vqvae_compression_audio_tactile_amd import _lib
    S, BLOCK = S_POOL, 2 * CAP
    gen = torch.Generator(device="cpu").manual_seed(29)
    w, x_total = 4000, 2 * 640 + 2 * 320
    good = (2, 5120, 640, 3000, 0)                                                    # session 0 of every group, valid
    cases = {
        "slot == n_slots": (S, 5120, 320, 3000, 1280),
        "slot == -1": (-1, 5120, 320, 3000, 1280),
        "drop > fill + n": (1, 5120, 320, 5441, 1280),
        "x_off + 2n > x_total": (1, 5120, 320, 3000, 1281),
        "fill + n - drop > cap": (1, CAP, 320, 319, 1280),
        "w > fill + n": (1, 3000, 320, 0, 1280),
        "negative n": (1, 5120, -320, 0, 1280),
    }
    for name, badrow in cases.items():
        big0 = torch.randn((S + 2) * BLOCK, generator=gen).to(dev)
        xbig0 = torch.randn(BLOCK + x_total + BLOCK, generator=gen).to(dev)
        big, xbig = big0.clone(), xbig0.clone()
        pool, x = big[BLOCK:BLOCK + S * BLOCK], xbig[BLOCK:BLOCK + x_total]
        pool0 = big0[BLOCK:BLOCK + S * BLOCK].view(S, 2, CAP)
        out = _nan(2 * 2 * w + GUARD, dev)
        dd = torch.tensor([good, badrow], dtype=torch.int32, device=dev)
        rc = _lib.lib().mvq_stream_samples_slots_f32(pool.data_ptr(), dd.data_ptr(), 2, S, x.data_ptr(), x_total, out.data_ptr(), w, CAP,
                                                     _stream())
        assert rc == 0, name
        xs = [xbig0[BLOCK:BLOCK + 1280].view(2, 640)]
        want_win, want_pool = _reference(pool0, [2], [(5120, 640, 3000)], xs, w)
        got = out[:4 * w].view(2, 2, w)
        assert torch.equal(got[:, 0], want_win[:, 0]), name                           # the valid session of the group is served
        assert not got[:, 1].any(), name                                              # both window rows of the other: zeros
        assert bool(torch.isnan(out[4 * w:]).all()), name
        assert torch.equal(pool.view(S, 2, CAP), want_pool), name                     # nothing stored for it
        assert torch.equal(big[:BLOCK], big0[:BLOCK]) and torch.equal(big[-BLOCK:], big0[-BLOCK:]), name
        assert torch.equal(xbig, xbig0), name


# ------------------------------------------------------------------------------------------------------- 3. end to end
OPENS = [0, 0, 1, 2, 3]                                                                # the tick each session opens at


def _patterns():
    return [sn.split_pushes(LENGTHS[0], 16), [8] + sn.split_pushes(LENGTHS[1] - 8 * 320, 16), sn.split_pushes(LENGTHS[2], "mixed", seed=9),
            sn.split_pushes(LENGTHS[3], 1), sn.split_pushes(LENGTHS[4], "mixed", seed=5)]


def _drive(pool, signals, patterns, opens, host=None):
    """Run the sessions through ``pool``, session i opening at tick opens[i]: each tick pushes the next piece of every open
    session's pattern and finishes the ones whose pattern is used up (with whatever samples remain).
    ``host``: None -- the even sessions push host tensors, the odd ones device tensors; True -- every push is a host tensor (the
    tick's samples then go up in one copy).
    -> (per session the outputs step by step, its StreamInfo, its slot), per tick (the groups, {sid: fill before the tick})."""
    n_s = len(signals)
    sids, pos, k, slot = {}, {}, {}, {}
    outs, infos, done, ticks = {i: [] for i in range(n_s)}, {}, set(), []
    tick = 0
    while len(done) < n_s:
        for i, t0 in enumerate(opens):
            if t0 == tick:
                sids[i], pos[i], k[i] = pool.open(), 0, 0
                slot[i] = pool._sess[sids[i]][0]
        pushes, finishes = {}, {}
        for i, sid in sids.items():
            if i in done:
                continue
            a, t = signals[i]
            if k[i] < len(patterns[i]):
                n = 320 * patterns[i][k[i]]
                piece = (a[..., pos[i]:pos[i] + n], t[..., pos[i]:pos[i] + n])
                pushes[sid] = piece if i % 2 and not host else tuple(p.cpu() for p in piece)
                pos[i] += n
            else:
                finishes[sid] = (a[..., pos[i]:], t[..., pos[i]:]) if pos[i] < a.shape[-1] else None
        before = {sid: pool._sess[sid][1] for sid in list(pushes) + list(finishes)}
        out = pool.step(pushes, finishes)
        assert sorted(out) == sorted(list(pushes) + list(finishes))
        ticks.append((pool.last_groups, before))
        for i, sid in sids.items():
            if sid in pushes:
                k[i] += 1
                pk, codes = out[sid]
                outs[i].append(([pk], codes))
                assert pool.tokens(sid) == pos[i] // 320
            elif sid in finishes:
                pk, codes, infos[i] = out[sid]
                outs[i].append(([pk], codes))
                done.add(i)
        tick += 1
    return outs, infos, slot, ticks


def test_sender_pool_equals_compress_packets_per_session(dev):
    from multimodal_vqvae_compression_audio_tactile_amd import MvqError
    net = _net(dev)
    refs = [_case(dev, 1, L) for L in LENGTHS]
    patterns = _patterns()
    assert len(patterns[2]) == 1 and patterns[1] == [8, 16] and set(patterns[3]) == {1}
    pool = net.stream_sender_pool(slots=4)
    outs, infos, slot, ticks = _drive(pool, [r[:2] for r in refs], patterns, OPENS)
    assert pool.active == () and pool.free == 4
    assert len({slot[i] for i in range(4)}) == 4 and slot[4] == min(slot[1], slot[2])   # the fifth reuses the lowest slot freed at tick 2
    assert pool.buf[slot[4]].any() and pool.carry[slot[4]].any()
    for i, ref in enumerate(refs):
        _check_session(outs[i], infos[i], 1, ref, patterns[i])                       # packets, codes, StreamInfo, emit counts
        assert all(isinstance(p, bytes) for step in outs[i] for p in step[0][0])
        assert all(step[1].shape[:2] == (1, 32) and step[1].dtype == torch.int64 for step in outs[i])
    # a group of two or more sessions that entered the tick with unequal fill ...
    mixed = [g for groups, before in ticks for g in groups if g.hi > g.lo and len({before[s] for s in g.sids}) > 1]
    assert mixed and any(g.key == ("emit", 0) for g in mixed)
    groups1, before1 = ticks[1]
    assert [g.key for g in groups1][-1] == ("emit", 0) and groups1[-1].sids == (0, 1) and (before1[0], before1[1]) == (16 * 320, 8 * 320)
    # ... and a tick with an append group and an emitting group together
    assert any(groups[0].key == ("append",) and any(g.hi > g.lo for g in groups[1:]) for groups, _ in ticks if groups)
    with pytest.raises(MvqError, match="no open session"):
        pool.step({0: (refs[0][0][..., :320], refs[0][1][..., :320])})


def test_steady_group_mixes_sessions_of_different_fill(dev):
    """One item fed as [16, 16, 16, 16] and as [8, 16, 16, 16, 16]: from tick 1 on the two sessions emit together, holding 16 / 8
    tokens at chunk 0 and 24 / 16 in the steady state, and each equals the item's compress_packets."""
    net = _net(dev)
    ref = _case(dev, 1, LENGTHS[0])
    patterns = [[16] * 4, [8] + [16] * 4]
    pool = net.stream_sender_pool(slots=2)
    outs, infos, _, ticks = _drive(pool, [ref[:2], ref[:2]], patterns, [0, 0])
    for i in range(2):
        _check_session(outs[i], infos[i], 1, ref, patterns[i])
    for tick, key, fills in ((1, ("emit", 0), (16, 8)), (2, ("emit", 1), (24, 16)), (3, ("emit", 1), (24, 16))):
        groups, before = ticks[tick]
        assert [g.key for g in groups] == [key] and groups[0].sids == (0, 1)
        assert (before[0], before[1]) == (320 * fills[0], 320 * fills[1])


# ----------------------------------------------------------------------------------------------- 4. pool against solo
@pytest.mark.parametrize("ptok,use", [(4, None), (16, 3)])
def test_a_pool_session_equals_a_solo_sender_step_by_step(ptok, use, dev):
    net = _net(dev)
    signals = [_case(dev, 1, L)[:2] for L in (LENGTHS[1], LENGTHS[4])]
    patterns = [sn.split_pushes(LENGTHS[1], "mixed", seed=2), sn.split_pushes(LENGTHS[4], "mixed", seed=5)]
    pool = net.stream_sender_pool(packet_tok=ptok, slots=2, books_use=use)
    outs, infos, _, _ = _drive(pool, signals, patterns, [0, 1], host=True if ptok == 4 else None)
    for i, (a, t) in enumerate(signals):
        tx = net.stream_sender(packet_tok=ptok, batch=1, books_use=use)
        pos = 0
        for j, m in enumerate(patterns[i]):
            pk, codes = tx.push(a[..., pos:pos + 320 * m], t[..., pos:pos + 320 * m])
            pos += 320 * m
            assert outs[i][j][0] == pk and outs[i][j][1].shape == codes.shape and torch.equal(outs[i][j][1], codes), (i, j)
        pk, codes, info = tx.finish(a[..., pos:], t[..., pos:]) if pos < a.shape[-1] else tx.finish()
        assert len(outs[i]) == len(patterns[i]) + 1
        assert outs[i][-1][0] == pk and torch.equal(outs[i][-1][1], codes) and infos[i] == info
        assert info.nb == (8 if use is None else use) and info.packet_tok == ptok
        assert any(step[0][0] for step in outs[i][:-1])                               # pushes did emit


# ---------------------------------------------------------------------------------------------------- 5. both pools
@pytest.mark.parametrize("name", ["alternating", "thin1"])
def test_sender_pool_into_receiver_pool_equals_the_whole_item_link(name, dev):
    net = _net(dev)
    Ls = [LENGTHS[0], LENGTHS[1], LENGTHS[4]]                                          # 75 / 37 / 39 tokens
    refs = [_case(dev, 1, L) for L in Ls]
    wants = []
    for i, (a, t, infos, pk, codes) in enumerate(refs):
        aud = [bitstream.pack_indices(codes[0].numpy(), 1024)]
        wants.append(net.decompress_packets(infos, [_channel(pk[0], i, name, infos[0])], aud)[0])
    tx, rx = net.stream_sender_pool(slots=3), net.stream_receiver_pool(512, 8, slots=3)
    patterns = [sn.split_pushes(L, "mixed", seed=3 + i) for i, L in enumerate(Ls)]
    opens = [0, 1, 2]
    txs, rxs, pos, k = {}, {}, {}, {}
    pend_pk, pend_codes, ended = {i: [] for i in range(3)}, {}, set()
    ys, closed = {i: [] for i in range(3)}, set()
    tick = 0
    while len(closed) < 3:
        for i, t0 in enumerate(opens):
            if t0 == tick:
                txs[i], rxs[i], pos[i], k[i] = tx.open(), rx.open(), 0, 0
                pend_codes[i] = torch.empty(1, 32, 0, dtype=torch.int64, device=dev)
        pushes, finishes = {}, {}
        for i in txs:
            if i in ended:
                continue
            a, t = refs[i][:2]
            if k[i] < len(patterns[i]):
                n = 320 * patterns[i][k[i]]
                pushes[txs[i]] = (a[..., pos[i]:pos[i] + n], t[..., pos[i]:pos[i] + n])
                pos[i], k[i] = pos[i] + n, k[i] + 1
            else:
                finishes[txs[i]] = (a[..., pos[i]:], t[..., pos[i]:]) if pos[i] < a.shape[-1] else None
        out = tx.step(pushes, finishes)
        for i in txs:                                                                  # the channel, per session
            if txs[i] in out:
                pend_pk[i] += _channel(out[txs[i]][0], i, name, refs[i][2][0])
                pend_codes[i] = torch.cat([pend_codes[i], out[txs[i]][1]], dim=2)
                if txs[i] in finishes:
                    assert out[txs[i]][2] == refs[i][2][0]
                    ended.add(i)
        while True:                                                                    # the receiver pool: a chunk per session and step
            r_push, r_fin = {}, {}
            for i in rxs:
                if i in closed:
                    continue
                lo_seq = rx.tokens(rxs[i]) // 2
                have = pend_codes[i]
                if have.shape[2] >= 16:
                    r_push[rxs[i]] = ([p for p in pend_pk[i] if lo_seq <= _seq(p) < lo_seq + 8], have[..., :16])
                    pend_codes[i] = have[..., 16:]
                elif i in ended:
                    r_fin[rxs[i]] = ([p for p in pend_pk[i] if _seq(p) >= lo_seq], have[0]) if have.shape[2] else None
                    closed.add(i)
            if not r_push and not r_fin:
                break
            y = rx.step(r_push, r_fin)
            for i in rxs:
                if rxs[i] in y:
                    ys[i].append(y[rxs[i]])
        tick += 1
    for i in range(3):
        got = torch.cat(ys[i], dim=-1)
        assert got.shape == wants[i].shape == (1, 1, 320 * refs[i][2][0].T - 8) and torch.equal(got, wants[i]), i


# ----------------------------------------------------------------------------------------------------------- 6. refusals
def test_sender_pool_refusals_on_the_device(dev):
    from multimodal_vqvae_compression_audio_tactile_amd import MvqError, ops
    net = _net(dev)
    with pytest.raises(ValueError, match="does not divide"):
        net.stream_sender_pool(packet_tok=3)
    with pytest.raises(ValueError, match="slots"):
        net.stream_sender_pool(slots=0)
    pool = net.stream_sender_pool(slots=3)
    a, b, c = pool.open(), pool.open(), pool.open()
    with pytest.raises(MvqError, match="all 3 slots"):
        pool.open()
    g = torch.Generator(device="cpu").manual_seed(5)
    x = (0.3 * torch.randn(1, 1, 5120, generator=g)).to(dev)
    pool.step({a: (x, x), b: (x[..., :2560], x[..., :2560]), c: (x, x)})              # a state worth comparing
    pool.step({a: (x, x)})                                                            # a has emitted chunk 0: a carried token
    assert pool.buf.any() and pool.carry.any()
    buf0, carry0 = pool.buf.clone(), pool.carry.clone()
    sess0 = {sid: list(v) for sid, v in pool._sess.items()}
    good = (x, x)
    with pytest.raises(MvqError, match="no open session 7"):
        pool.step({a: good, b: good, 7: good})
    with pytest.raises(ValueError, match="both"):
        pool.step({a: good, b: good}, {b: None})
    with pytest.raises(ValueError, match="1 <= m <= 16"):
        pool.step({a: good, b: (x[..., :100], x[..., :100]), c: good})
    with pytest.raises(ValueError, match="1 <= m <= 16"):
        x17 = torch.zeros(1, 1, 5440, device=dev)
        pool.step({a: good, b: good, c: (x17, x17)})
    with pytest.raises(ValueError, match="advance together"):
        pool.step({a: good, b: (x, x[..., :320]), c: good})
    with pytest.raises(ValueError, match="advance together"):
        pool.step({a: good}, {b: (x, x[..., :100]), c: None})
    with pytest.raises(ValueError, match="needs its samples"):
        pool.step({a: good, b: None, c: good})
    with pytest.raises(ValueError, match="batch"):
        pool.step({a: good, b: (torch.cat([x, x]), torch.cat([x, x])), c: good})
    with ops.arith("f16x3"):
        with pytest.raises(ValueError, match="arithmetic"):
            pool.step({a: good, b: good, c: good})
        with pytest.raises(ValueError, match="arithmetic"):
            net.stream_sender_pool()
    torch.cuda.synchronize()
    assert torch.equal(pool.buf, buf0) and torch.equal(pool.carry, carry0)            # nothing ran, nothing moved
    assert {sid: list(v) for sid, v in pool._sess.items()} == sess0 and pool.active == (a, b, c) and pool.free == 0
    # the sessions go on, and a finished or closed one is gone
    out = pool.step({a: good}, {b: None})
    assert len(out[a][0]) == 8 and out[a][1].shape == (1, 32, 16) and pool.tokens(a) == 48
    assert len(out[b][0]) == 4 and out[b][1].shape == (1, 32, 8) and out[b][2] == StreamInfo(512, 8, 8, 2)
    pool.close(c)
    assert pool.active == (a,) and pool.free == 2
    for gone in (b, c):
        with pytest.raises(MvqError, match="no open session"):
            pool.step({gone: good})
        with pytest.raises(MvqError, match="no open session"):
            pool.step({}, {gone: None})
        with pytest.raises(MvqError, match="no open session"):
            pool.close(gone)
    # an item shorter than a token: nothing to send and no device work
    d = pool.open()
    assert d == 3 and pool._sess[d][0] == 1                                           # a new sid, the lowest free slot
    out = pool.step({}, {d: (x[..., :100], x[..., :100])})
    assert out[d][0] == [] and out[d][1].shape == (1, 32, 0) and out[d][2] == StreamInfo(512, 8, 0, 2)
    assert pool.step({}) == {}
