"""-m gpu: the pools for the whole link on the device --
  1. mvq_hold_fill_slots_f32 against the numpy hold_fill (tests/audio_conceal_oracle.py), bit for bit;
  2. StreamReceiverPoolAV per session, call by call, against StreamReceiver(batch=1) with the same options, and concatenated
     against decompress_packets_av of that item alone;
  3. StreamSenderPoolAV per session, step by step, against StreamSender(batch=1), and per item against compress_packets(_av);
  4. sender pool -> the lossy channel on both streams and their parity -> receiver pool against the whole-item link;
  5. the refusals of a tick, each of which leaves every session as it was.
Every comparison is an equality.  The model and the signals are those of tests/test_gpu_sender.py / test_gpu_stream.py; the loss is a
fixed function of (session, sequence number), so the whole-item calls and the chunk-by-chunk sessions see the same channel, and the
host-side numpy rule (packets.fec_recover) says what it does to every parity group before anything is decoded."""
import numpy as np
import pytest
import torch

import audio_conceal_oracle as ac
import sender_oracle as sn
from multimodal_vqvae_compression_audio_tactile_amd import packets, stream
from multimodal_vqvae_compression_audio_tactile_amd.packets import Fec, Rate, StreamInfo
from fec_rs_channel import seq_of
from test_gpu_sender import LENGTHS, _net, _stream
from test_gpu_sender import _case as _sender_case
from test_gpu_sender_pool import OPENS as TX_OPENS
from test_gpu_sender_pool import _patterns
from test_gpu_stream_pool import ITEMS, LISTS, OPENS, S_POOL

pytestmark = pytest.mark.gpu

f32 = np.float32
GUARD = 64
RATE, ARATE = Rate(min_books=2, tol2=0.84), Rate(min_books=2, tol2=0.5)      # tests/test_gpu_rate.py, tests/test_gpu_av.py
FEC, AFEC = Fec(4, 3), Fec(8, 4, 2)
TOKENS = [T for T, _ in ITEMS]                                               # 75 / 37 / 16 / 11 / 40
_REF = {}


def _bits(x):
    return np.ascontiguousarray(x, f32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------- 1. the slot kernel
@pytest.mark.parametrize("C,T", [(20, 1), (96, 130), (1024, 37)])
def test_hold_fill_slots_kernel_equals_numpy(C, T, dev):
    from multimodal_vqvae_compression_audio_tactile_amd import MvqError, _lib, ops
    S = S_POOL
    r = np.random.default_rng(C + T)
    lib = _lib.lib()
    nan = lambda n: torch.full((n,), float("nan"), device=dev)

    def inputs(G):
        x = r.standard_normal((G, C, T)).astype(f32)
        x.reshape(-1)[::7] = -0.0
        xb = _bits(x)
        xb.reshape(-1)[5::13] = 0x7FC12345                                   # NaNs with a payload
        xb.reshape(-1)[6::17] = 0xFF800000                                   # -inf
        pool = r.standard_normal((S, C)).astype(f32)
        pool[0, 0] = -0.0
        _bits(pool).reshape(-1)[3::11] = 0x7FC00077
        pats = {"none": np.zeros((G, T), np.uint8), "all": np.full((G, T), 32, np.uint8),
                "runs": np.tile(((np.arange(T) // 3) % 2).astype(np.uint8), (G, 1))}
        per = (r.uniform(size=(G, T)) < 0.4).astype(np.uint8)
        per[0] = 0                                                           # item 0 all lost
        pats["per_item"] = per
        if T > 64:
            far = np.zeros((G, T), np.uint8)
            far[:, 3] = 1
            far[:, 64] = 1                                                   # a source two tiles back; one at a tile's first lane
            pats["far"] = far
        return xb.view(f32), pool, pats

    def run(x, valid, pool, slots_dev, G):
        """The C entry point on guarded copies -> (x bits, pool bits); the guard bands stay NaN."""
        xbuf = torch.cat([torch.from_numpy(x).to(dev).reshape(-1), nan(GUARD)])
        pbuf = torch.cat([torch.from_numpy(pool).to(dev).reshape(-1), nan(GUARD)])
        vd = torch.from_numpy(valid).to(dev)
        assert lib.mvq_hold_fill_slots_f32(xbuf.data_ptr(), vd.data_ptr(), pbuf.data_ptr(), slots_dev.data_ptr(), G, S, C, T, _stream()) == 0
        assert bool(torch.isnan(xbuf[G * C * T:]).all()) and bool(torch.isnan(pbuf[S * C:]).all())
        return _bits(xbuf[:G * C * T].cpu().numpy().reshape(G, C, T)), _bits(pbuf[:S * C].cpu().numpy().reshape(S, C))

    for slots in LISTS + [list(range(S))]:
        G = len(slots)
        x, pool, pats = inputs(G)
        sd = torch.tensor(slots, dtype=torch.int32, device=dev)
        for name, valid in pats.items():
            want, want_rows = ac.hold_fill(x, valid, pool[slots])
            want_pool = pool.copy()
            want_pool[slots] = want_rows                                     # unlisted rows: bit-identical to before
            got_x, got_pool = run(x, valid, pool, sd, G)
            assert np.array_equal(got_x, _bits(want)) and np.array_equal(got_pool, _bits(want_pool)), (slots, name)
            for kw in (dict(slots=slots), dict(slots=slots, slots_dev=sd)):  # the wrapper, the list uploaded by it or by the caller
                xd, vd, pd = torch.from_numpy(x.copy()).to(dev), torch.from_numpy(valid).to(dev), torch.from_numpy(pool.copy()).to(dev)
                assert ops.hold_fill_(xd, vd, pd, **kw) is xd
                assert np.array_equal(_bits(xd.cpu().numpy()), _bits(want)) and np.array_equal(_bits(pd.cpu().numpy()), _bits(want_pool))
            if G == S:                                                       # the identity list equals the dense call
                xd, vd, pd = torch.from_numpy(x.copy()).to(dev), torch.from_numpy(valid).to(dev), torch.from_numpy(pool.copy()).to(dev)
                ops.hold_fill_(xd, vd, pd)
                assert np.array_equal(_bits(xd.cpu().numpy()), got_x) and np.array_equal(_bits(pd.cpu().numpy()), got_pool), name
    # the kernel's own range check (the wrapper never lets such a list through): +0 is read as the carry, no carry is stored
    x, pool, pats = inputs(2)
    bad = torch.tensor([S, -1], dtype=torch.int32, device=dev)
    for name in ("none", "per_item", "runs"):
        got_x, got_pool = run(x, pats[name], pool, bad, 2)
        assert np.array_equal(got_x, _bits(ac.hold_fill(x, pats[name])[0])) and np.array_equal(got_pool, _bits(pool)), name
    xd, vd, pd = torch.from_numpy(x.copy()).to(dev), torch.from_numpy(pats["runs"]).to(dev), torch.from_numpy(pool.copy()).to(dev)
    for slots, what in (([0, S], "outside"), ([-1, 0], "outside"), ([2, 2], "twice"), ([0], "1 slots"), (torch.tensor([0, 1]), "host integers")):
        with pytest.raises(MvqError, match=what):
            ops.hold_fill_(xd, vd, pd, slots=slots)
    with pytest.raises(MvqError, match="slots_dev"):
        ops.hold_fill_(xd, vd, pd, slots=[0, 1], slots_dev=torch.tensor([0, 1], device=dev))
    with pytest.raises(MvqError, match="host list"):
        ops.hold_fill_(xd, vd, pd, slots_dev=torch.tensor([0, 1], dtype=torch.int32, device=dev))
    with pytest.raises(MvqError, match="pool"):
        ops.hold_fill_(xd, vd, torch.zeros(S, C + 1, device=dev), slots=[0, 1])
    torch.cuda.synchronize()
    assert np.array_equal(_bits(xd.cpu().numpy()), _bits(x)) and np.array_equal(_bits(pd.cpu().numpy()), _bits(pool))   # nothing ran


# ------------------------------------------------------------------------------------------------------------ the channel
def _lose(i, pk, par, info, fec, audio):
    """The channel of session ``i`` on one stream, a fixed function of the sequence number -> (what arrives, the parity that
    arrives), both reversed.  Tactile (groups of 4, one parity packet), group j: j % 4 == 0 loses its first packet; 1 loses two
    (more than its parity); 2 loses its last packet AND its parity; 3 has, for even i, its second packet thinned to one book.
    Audio (groups of 8 = a chunk, two parity packets), chunk c: c % 4 == 0 loses its first packet and, for even i, both parity
    packets; 1 loses its first three packets; 2 loses one packet and parity 0; 3 loses two packets."""
    drop, thin, plost = set(), {}, set()
    g, r = int(fec.group), fec.r
    for j in range((info.P + g - 1) // g):
        m = j % 4
        if audio:
            drop |= set([(g * j,), (g * j, g * j + 1, g * j + 2), (g * j + (i + 3) % 8,), (g * j + 2, g * j + 5)][m])
            if m == 0 and i % 2 == 0:
                plost |= {r * j, r * j + 1}
            if m == 2:
                plost.add(r * j)
        else:
            drop |= set([(g * j,), (g * j + 1, g * j + 2), (g * j + 3,), ()][m])
            if m == 2:
                plost.add(j)
            if m == 3 and i % 2 == 0 and g * j + 1 < info.P:
                thin[g * j + 1] = 1
    rx = [packets.thin(p, thin[s], info) if s in thin else p for s, p in enumerate(pk) if s not in drop]
    return rx[::-1], [p for k, p in enumerate(par) if k not in plost][::-1]


def _what_the_rule_does(rx, rxp, pk, par, info, fec):
    """packets.fec_recover on the host -> (recovered any, a group with more deficient packets than arrived parity, a parity packet
    was lost, the counts per packet after recovery)."""
    bodies, counts = packets.gather(rx, info)
    rows, got = packets.gather_fec(rxp, info, fec)
    _, after, rec = packets.fec_recover(bodies, counts, rows, got, info, fec)
    g, m, G, _ = fec.resolve(info)
    sent = [p[8] for p in pk]
    too_many = False
    for j in range(G):
        grp = range(j * g, min(info.P, (j + 1) * g))
        deficient = sum(int(counts[p]) < min(m, sent[p]) for p in grp)
        arrived = bin(int(got[j])).count("1")
        too_many |= deficient > arrived
    return bool(rec.any()), too_many, len(rxp) < len(par), after


def _item(dev, i):
    """Session i's item, its packets of both streams and their parity (compress_packets_av), what arrives of each, and the
    whole-item results -- computed once and shared."""
    if ("item", i) not in _REF:
        from multimodal_vqvae_compression_audio_tactile_amd import synth
        net, T = _net(dev), TOKENS[i]
        L = 320 * T
        a, t = synth.audio_segments(1, seed=L % 1000 + 1, T=L).to(dev), synth.tactile_segments(1, seed=L % 1000 + 1, T=L).to(dev)
        infos, pk, ainfos, apk, par, apar = net.compress_packets_av(a, t, rate=RATE, audio_rate=ARATE, fec=FEC, audio_fec=AFEC)
        info, ainfo = infos[0], ainfos[0]
        assert (info.T, ainfo.T) == (T, T)
        rx, rxp = _lose(i, pk[0], par[0], info, FEC, False)
        arx, arxp = _lose(i, apk[0], apar[0], ainfo, AFEC, True)
        _REF[("item", i)] = dict(a=a, t=t, info=info, ainfo=ainfo, pk=pk[0], apk=apk[0], par=par[0], apar=apar[0], rx=rx, rxp=rxp, arx=arx,
                                 arxp=arxp, rule=_what_the_rule_does(rx, rxp, pk[0], par[0], info, FEC),
                                 arule=_what_the_rule_does(arx, arxp, apk[0], apar[0], ainfo, AFEC))
    return _REF[("item", i)]


def test_the_channel_is_not_vacuous(dev):
    """On the host, with the numpy rule: every stream sees a recovered packet, a group beyond repair and a lost parity packet; the
    audio stream keeps a lost token at the first position of a later chunk, and a session's very first audio token stays lost."""
    items = [_item(dev, i) for i in range(len(TOKENS))]
    for key in ("rule", "arule"):
        assert any(it[key][0] for it in items) and any(it[key][1] for it in items) and any(it[key][2] for it in items), key
    assert any(it["arule"][3][8 * c] == 0 for it in items for c in range(1, it["ainfo"].T // 16)), "first token of a later chunk"
    assert any(it["arule"][3][0] == 0 for it in items), "a session's first audio token"
    assert any(it["arule"][3][0] != 0 for it in items)
    counts = packets.gather(items[0]["rx"], items[0]["info"])[1]             # and a tactile packet arrives thinned below its protection
    assert (counts == 0).any() and ((counts > 0) & (counts < [min(3, p[8]) for p in items[0]["pk"]])).any()


# ---------------------------------------------------------------------------------------------------- 2. the receiver pool
def _chunk_of(it, c, last, extra=False):
    """What arrives of chunk ``c`` (``last``: everything from it on) -> (tactile, audio, parity, audio parity); ``extra``: also a
    late data packet and a late parity packet of chunk 0 on each stream."""
    def pick(lst, per):
        return [p for p in lst if (seq_of(p) >= per * c if last else per * c <= seq_of(p) < per * (c + 1))]
    out = [pick(it["rx"], 8), pick(it["arx"], 8), pick(it["rxp"], 2), pick(it["arxp"], 1)]
    if extra:
        out = [out[0] + it["pk"][1:2], out[1] + it["apk"][3:4], out[2] + it["par"][:1], out[3] + it["apar"][1:2]]
    return out


def _solo(dev, i, kw):
    """StreamReceiver(batch=1) on session i's data -> its outputs call by call, its late count."""
    it, T = _item(dev, i), TOKENS[i]
    rx = _net(dev).stream_receiver(512, 8, batch=1, audio=(1024, 32), fec=FEC, audio_fec=AFEC, **kw)
    ys = []
    for c in range(T // 16):
        tp, ap, fp, afp = _chunk_of(it, c, False, extra=(i == 0 and c == 2))
        ys.append(rx.push([tp], audio_packets=[ap], fec_packets=[fp], audio_fec_packets=[afp]).clone())
    if T % 16:
        tp, ap, fp, afp = _chunk_of(it, T // 16, True)
        ys.append(rx.finish([tp], [ap], tokens=T % 16, fec_packets=[fp], audio_fec_packets=[afp]))
    else:
        ys.append(rx.finish())
    return ys, rx.late


def _drive_rx(pool, dev, sessions, opens, tuples=False):
    """The sessions (indices into TOKENS) through ``pool``, session k opening at tick opens[k]; each tick pushes the next full
    chunk of every open session and finishes the ones that have none left -> (outputs per session, late counts, slots)."""
    sids, nxt, done, slot = {}, {}, set(), {}
    outs, lates = {k: [] for k in range(len(sessions))}, {}
    tick = 0
    while len(done) < len(sessions):
        for k, t0 in enumerate(opens):
            if t0 == tick:
                sids[k], nxt[k] = pool.open(), 0
                slot[k] = pool._sess[sids[k]][0]
        pushes, finishes = {}, {}
        for k, sid in sids.items():
            if k in done:
                continue
            i = sessions[k]
            it, T, c = _item(dev, i), TOKENS[i], nxt[k]
            if 16 * (c + 1) <= T:
                parts = _chunk_of(it, c, False, extra=(i == 0 and c == 2))
                pushes[sid] = tuple(parts) if tuples or k % 2 else stream.PoolChunk(*parts)
            elif T % 16:
                finishes[sid] = stream.PoolChunk(*_chunk_of(it, c, True), tokens=T % 16)
            else:
                finishes[sid] = None
        out = pool.step(pushes, finishes)
        assert sorted(out) == sorted(list(pushes) + list(finishes))
        for k, sid in sids.items():
            if sid in out:
                outs[k].append(out[sid])
            if sid in pushes:
                nxt[k] += 1
                assert pool.tokens(sid) == 16 * nxt[k]
                lates[k] = pool.late(sid)
            elif sid in finishes:
                done.add(k)
        tick += 1
    return outs, lates, slot


RX_CASES = [("zero", "predict", 24000, "window"), ("mask", "predict", 24000, "window"), ("hold", "predict", 24000, "window"),
            ("hold", "zero", 24000, "window"), ("mask", "predict", 3000, "window"), ("hold", "predict", 24000, "stateful")]


@pytest.mark.parametrize("audio_conceal,conceal,out_rate,decoder", RX_CASES)
def test_receiver_pool_av_equals_the_solo_receiver_per_session(audio_conceal, conceal, out_rate, decoder, dev):
    from multimodal_vqvae_compression_audio_tactile_amd import Resample
    net = _net(dev)
    kw = dict(conceal=conceal, out_rate=out_rate, audio_conceal=audio_conceal, decoder=decoder)
    pool = net.stream_receiver_pool_av(512, 8, slots=4, audio=(1024, 32), fec=FEC, audio_fec=AFEC, **kw)
    assert type(pool) is stream.StreamReceiverPoolAV and (pool.qa_carry is not None) == (audio_conceal == "hold")
    for state in (pool.carry, pool.qa_carry, pool.rs_state):                 # a reset that open() misses shows
        if state is not None:
            state.fill_(float("nan"))
    outs, lates, slot = _drive_rx(pool, dev, list(range(5)), OPENS)
    assert pool.active == () and pool.free == 4
    assert slot[4] in (slot[1], slot[2], slot[3]) and len({slot[k] for k in range(4)}) == 4      # the fifth session reuses a freed slot
    for i, T in enumerate(TOKENS):
        it = _item(dev, i)
        ys, late = _solo(dev, i, kw)
        assert len(outs[i]) == len(ys)
        for j, (got, want) in enumerate(zip(outs[i], ys)):                   # call by call
            assert got.shape == want.shape and torch.equal(got, want), (i, j)
        if T >= 16:
            assert lates[i] == late == (4 if i == 0 else 0)                  # the four stragglers of session 0, counted for it alone
        key = ("whole", i, conceal, audio_conceal)
        if key not in _REF:
            _REF[key] = net.decompress_packets_av([it["info"]], [it["rx"]], [it["ainfo"]], [it["arx"]], conceal=conceal, fec=FEC,
                                                  fec_packets=[it["rxp"]], audio_fec=AFEC, audio_fec_packets=[it["arxp"]],
                                                  audio_conceal=audio_conceal)[0]
        want = _REF[key]
        assert want.shape == (1, 1, 320 * T - 8)
        if out_rate == 3000:
            want = Resample(24000, 3000).to(dev)(want)
        got = torch.cat(outs[i], dim=-1)
        print(f"rx pool session {i}: T={T} calls={len(outs[i])} samples={got.shape[-1]} sum|y|={float(got.abs().sum()):.6g} "
              f"finite={bool(torch.isfinite(got).all())} late={lates.get(i)} device={torch.cuda.get_device_name(got.device)}")
        assert got.shape == want.shape and torch.equal(got, want), i
    if audio_conceal != "zero":                                              # the mode did something on this channel
        plain = ("whole", 0, conceal, "zero")
        if plain in _REF:
            assert not torch.equal(_REF[plain], _REF[("whole", 0, conceal, audio_conceal)])


def test_receiver_pool_av_with_audio_codes_and_tactile_fec(dev):
    """audio=None: a tactile-only stream with fec= gets a pool too; the audio travels as codes."""
    net = _net(dev)
    pool = net.stream_receiver_pool_av(512, 8, slots=2, fec=FEC)
    sessions = [1, 4]
    sids = {k: pool.open() for k in range(2)}
    solo = {k: net.stream_receiver(512, 8, batch=1, fec=FEC) for k in range(2)}
    codes = {}
    for k, i in enumerate(sessions):
        it = _item(dev, i)
        codes[k] = torch.from_numpy(np.asarray(packets.unpack_bodies(*packets.gather(it["apk"], it["ainfo"]), it["ainfo"])[0])).to(dev)
        assert codes[k].shape == (32, TOKENS[i])
    for c in range(3):
        pushes, finishes = {}, {}
        for k, i in enumerate(sessions):
            it, T = _item(dev, i), TOKENS[i]
            if sids[k] not in pool.active:
                continue
            last = 16 * (c + 1) > T
            tp, _, fp, _ = _chunk_of(it, c, last)
            (finishes if last else pushes)[sids[k]] = (tp, codes[k][:, 16 * c:16 * c + 16], fp)
        out = pool.step(pushes, finishes)
        for k, i in enumerate(sessions):
            if sids[k] in out:
                tp, cd, fp = (pushes if sids[k] in pushes else finishes)[sids[k]]
                want = solo[k].push([tp], cd[None], fec_packets=[fp]) if sids[k] in pushes else solo[k].finish([tp], cd[None], fec_packets=[fp])
                assert torch.equal(out[sids[k]], want), (k, c)
    assert pool.active == ()


# ------------------------------------------------------------------------------------------------------ 3. the sender pool
TX_CASES = {
    "av_fec": dict(rate=RATE, audio="packets", audio_rate=ARATE, fec=FEC, audio_fec=AFEC),
    "nine_stages": dict(audio="packets", audio_books=9),
    "codes_rate_fec": dict(audio="codes", rate=RATE, fec=FEC),
    "av_fec_stateful": dict(rate=RATE, audio="packets", audio_rate=ARATE, fec=FEC, audio_fec=AFEC, encoder="stateful"),
}


def _drive_tx(pool, signals, patterns, opens):
    """The sessions through ``pool`` as tests/test_gpu_sender_pool.py drives them (even sessions push host tensors, odd ones device
    tensors) -> per session what ``step`` returned for it, tick by tick."""
    n_s = len(signals)
    sids, pos, k, outs, done = {}, {}, {}, {i: [] for i in range(n_s)}, set()
    tick = 0
    while len(done) < n_s:
        for i, t0 in enumerate(opens):
            if t0 == tick:
                sids[i], pos[i], k[i] = pool.open(), 0, 0
        pushes, finishes = {}, {}
        for i, sid in sids.items():
            if i in done:
                continue
            a, t = signals[i]
            if k[i] < len(patterns[i]):
                n = 320 * patterns[i][k[i]]
                piece = (a[..., pos[i]:pos[i] + n], t[..., pos[i]:pos[i] + n])
                pushes[sid] = piece if i % 2 else tuple(p.cpu() for p in piece)
                pos[i], k[i] = pos[i] + n, k[i] + 1
            else:
                finishes[sid] = (a[..., pos[i]:], t[..., pos[i]:]) if pos[i] < a.shape[-1] else None
        out = pool.step(pushes, finishes)
        assert sorted(out) == sorted(list(pushes) + list(finishes))
        for i, sid in sids.items():
            if sid in out:
                outs[i].append(out[sid])
                if sid in finishes:
                    done.add(i)
                else:
                    assert pool.tokens(sid) == pos[i] // 320
        tick += 1
    return outs


def _same(pool_val, solo_val):
    """The pool returns the one item's values where the lockstep sender returns lists of one."""
    if isinstance(solo_val, torch.Tensor):
        return isinstance(pool_val, torch.Tensor) and pool_val.shape == solo_val.shape and pool_val.dtype == solo_val.dtype \
            and torch.equal(pool_val, solo_val)
    if isinstance(solo_val, StreamInfo):
        return pool_val == solo_val
    return isinstance(solo_val, list) and len(solo_val) == 1 and pool_val == solo_val[0] and all(isinstance(p, bytes) for p in pool_val)


@pytest.mark.parametrize("name", list(TX_CASES))
def test_sender_pool_av_equals_the_solo_sender_per_session(name, dev):
    net, kw = _net(dev), TX_CASES[name]
    signals = [_sender_case(dev, 1, L)[:2] for L in LENGTHS]
    patterns = _patterns()
    pool = net.stream_sender_pool_av(slots=4, **kw)
    assert type(pool) is stream.StreamSenderPoolAV
    pool.carry.fill_(float("nan"))                                           # a reset that open() misses shows
    outs = _drive_tx(pool, signals, patterns, TX_OPENS)
    assert pool.active == () and pool.free == 4
    n_data = 2
    for i, (a, t) in enumerate(signals):
        tx = net.stream_sender(batch=1, **kw)
        pos, solo = 0, []
        for m in patterns[i]:
            solo.append(tx.push(a[..., pos:pos + 320 * m], t[..., pos:pos + 320 * m]))
            pos += 320 * m
        solo.append(tx.finish(a[..., pos:], t[..., pos:]) if pos < a.shape[-1] else tx.finish())
        assert len(outs[i]) == len(solo)
        print(f"tx pool session {i}: steps={len(solo)} packets={sum(len(s_[0]) for s_ in outs[i])} "
              f"bytes={sum(len(p) for s_ in outs[i] for p in s_[0])}")
        for j, (got, want) in enumerate(zip(outs[i], solo)):                 # step by step
            assert len(got) == len(want) and all(_same(g, w) for g, w in zip(got, want)), (i, j)
        # per item: the concatenation is the whole-item call's
        fin = outs[i][-1]
        if kw["audio"] == "packets":
            n_info = 2
            whole = net.compress_packets_av(a, t, rate=kw.get("rate"), audio_books=kw.get("audio_books"), audio_rate=kw.get("audio_rate"),
                                            fec=kw.get("fec"), audio_fec=kw.get("audio_fec"))
            infos, pk, ainfos, apk = whole[:4]
            assert fin[2:4] == (infos[0], ainfos[0])
            lists = [pk[0], apk[0]] + ([whole[4][0], whole[5][0]] if len(whole) > 4 else [])
            cols = [0, 1] + ([2, 3] if len(whole) > 4 else [])
        else:
            n_info = 1
            whole = net.compress_packets(a, t, rate=kw.get("rate"), fec=kw.get("fec"))
            assert fin[2] == whole[0][0]
            lists, cols = [whole[1][0], whole[3][0]], [0, 2]
        steps = [s for s in outs[i][:-1]] + [fin[:n_data] + fin[n_data + n_info:]]
        for col, want in zip(cols, lists):
            assert sum((s[col] for s in steps), []) == want, (i, col)
        if kw["audio"] == "packets" and kw.get("audio_books") == 9:
            assert fin[3].nb == 9


# ----------------------------------------------------------------------------------------------------------- 4. the link
def _link(dev, lengths, opens, seeds, chan=None):
    """StreamSenderPoolAV -> the channel per session on both streams and their parity -> StreamReceiverPoolAV.
    -> per session the receiver's outputs call by call, and what its sender sent (packets, audio packets, parity, audio parity,
    StreamInfo, audio StreamInfo)."""
    net = _net(dev)
    n_s = len(lengths)
    chan = list(range(n_s)) if chan is None else chan                        # the channel each session goes through
    opts = dict(rate=RATE, audio="packets", audio_rate=ARATE, fec=FEC, audio_fec=AFEC)
    tx = net.stream_sender_pool_av(slots=n_s, **opts)
    rx = net.stream_receiver_pool_av(512, 8, slots=n_s, audio=(1024, 32), fec=FEC, audio_fec=AFEC, audio_conceal="hold")
    refs = [_sender_case(dev, 1, L) for L in lengths]
    patterns = [sn.split_pushes(L, "mixed", seed=s) for L, s in zip(lengths, seeds)]
    txs, rxs, pos, k = {}, {}, {}, {}
    sent = {i: [[], [], [], []] for i in range(n_s)}
    infos, sent_tok, ys, closed = {}, {i: 0 for i in range(n_s)}, {i: [] for i in range(n_s)}, set()
    tick = 0
    while len(closed) < n_s:
        for i, t0 in enumerate(opens):
            if t0 == tick:
                txs[i], rxs[i], pos[i], k[i] = tx.open(), rx.open(), 0, 0
        pushes, finishes = {}, {}
        for i in txs:
            if i in infos:
                continue
            a, t = refs[i][:2]
            if k[i] < len(patterns[i]):
                n = 320 * patterns[i][k[i]]
                pushes[txs[i]] = (a[..., pos[i]:pos[i] + n], t[..., pos[i]:pos[i] + n])
                pos[i], k[i] = pos[i] + n, k[i] + 1
            else:
                finishes[txs[i]] = (a[..., pos[i]:], t[..., pos[i]:]) if pos[i] < a.shape[-1] else None
        out = tx.step(pushes, finishes)
        for i in txs:
            o = out.get(txs[i])
            if o is None:
                continue
            data = o[:2] + (o[4:] if txs[i] in finishes else o[2:])
            for col in range(4):
                sent[i][col] += data[col]
            if txs[i] in finishes:
                infos[i] = o[2:4]
                sent_tok[i] = o[2].T
            elif o[0]:
                sent_tok[i] += 16
        while True:                                                          # the receiver pool: a chunk per session and step
            r_push, r_fin = {}, {}
            for i in rxs:
                if i in closed:
                    continue
                have, T = rx.tokens(rxs[i]), sent_tok[i]
                c = have // 16
                if i in infos:
                    info, ainfo = infos[i]
                else:                                                        # the stream so far: the chunks sent are whole
                    info, ainfo = StreamInfo(512, 8, T, 2), StreamInfo(1024, 32, T, 2)
                arrived = [_lose(chan[i], sent[i][0], sent[i][2], info, FEC, False), _lose(chan[i], sent[i][1], sent[i][3], ainfo, AFEC, True)]
                it = dict(rx=arrived[0][0], rxp=arrived[0][1], arx=arrived[1][0], arxp=arrived[1][1])
                if have + 16 <= T:
                    r_push[rxs[i]] = stream.PoolChunk(*_chunk_of(it, c, False))
                elif i in infos:
                    r_fin[rxs[i]] = stream.PoolChunk(*_chunk_of(it, c, True), tokens=T - have) if T > have else None
                    closed.add(i)
            if not r_push and not r_fin:
                break
            y = rx.step(r_push, r_fin)
            for i in rxs:
                if rxs[i] in y:
                    ys[i].append(y[rxs[i]])
        tick += 1
    return ys, sent, infos, refs


def test_sender_pool_av_into_receiver_pool_av_equals_the_whole_item_link(dev):
    net = _net(dev)
    lengths = [LENGTHS[0], LENGTHS[1], LENGTHS[4]]                           # 75 / 37 / 40 tokens
    ys, sent, infos, refs = _link(dev, lengths, [0, 1, 2], [3, 4, 5])
    for i, (a, t, *_) in enumerate(refs):
        w_infos, pk, w_ainfos, apk, par, apar = net.compress_packets_av(a, t, rate=RATE, audio_rate=ARATE, fec=FEC, audio_fec=AFEC)
        assert infos[i] == (w_infos[0], w_ainfos[0]) and sent[i] == [pk[0], apk[0], par[0], apar[0]]
        rx, rxp = _lose(i, pk[0], par[0], w_infos[0], FEC, False)
        arx, arxp = _lose(i, apk[0], apar[0], w_ainfos[0], AFEC, True)
        want = net.decompress_packets_av(w_infos, [rx], w_ainfos, [arx], fec=FEC, fec_packets=[rxp], audio_fec=AFEC, audio_fec_packets=[arxp],
                                         audio_conceal="hold")[0]
        got = torch.cat(ys[i], dim=-1)
        assert got.shape == want.shape == (1, 1, 320 * w_infos[0].T - 8) and torch.equal(got, want), i
        assert not torch.equal(want, net.decompress_packets_av(w_infos, [rx], w_ainfos, [arx])[0])       # parity and hold did something
    # one item alone equals the same item among others
    alone, _, _, _ = _link(dev, [LENGTHS[1]], [0], [4], chan=[1])
    assert len(alone[0]) == len(ys[1]) and all(torch.equal(p, q) for p, q in zip(alone[0], ys[1]))


# ------------------------------------------------------------------------------------------------------------ 5. refusals
def test_pool_av_refusals_leave_every_session_as_it_was(dev):
    from multimodal_vqvae_compression_audio_tactile_amd import MvqError
    net = _net(dev)
    pool = net.stream_receiver_pool_av(512, 8, slots=2, audio=(1024, 32), audio_fec=AFEC, audio_conceal="hold")     # no fec= on the tactile stream
    solo = [net.stream_receiver(512, 8, batch=1, audio=(1024, 32), audio_fec=AFEC, audio_conceal="hold") for _ in range(2)]
    sessions = [1, 3]                                                        # 37 and 11 tokens
    its = [_item(dev, i) for i in sessions]
    a, b = pool.open(), pool.open()
    tp, ap, fp, afp = _chunk_of(its[0], 0, False)
    got = pool.step({a: (tp, ap, None, afp)})[a]
    assert torch.equal(got, solo[0].push([tp], audio_packets=[ap], audio_fec_packets=[afp]))
    torch.cuda.synchronize()
    state = [x.clone() for x in (pool.carry, pool.qa_carry, pool.hist)]
    sess = {sid: list(v) for sid, v in pool._sess.items()}
    tp1, ap1, fp1, afp1 = _chunk_of(its[0], 1, False)
    tpb, apb, fpb, afpb = _chunk_of(its[1], 0, True)
    good_a, good_b = (tp1, ap1, None, afp1), stream.PoolChunk(tpb, apb, None, afpb, tokens=11)
    with pytest.raises(ValueError, match="need a pool opened with fec="):   # parity packets without fec=
        pool.step({a: (tp1, ap1, fp1, afp1)}, {b: good_b})
    with pytest.raises(ValueError, match="tokens = None"):                   # tokens= missing on a finish with audio packets
        pool.step({a: good_a}, {b: (tpb, apb, None, afpb)})
    with pytest.raises(ValueError, match="both pushed and finished"):        # a sid in both maps
        pool.step({a: good_a, b: good_a}, {b: good_b})
    with pytest.raises(MvqError, match="StreamReceiverPoolAV: push: no open session 7"):
        pool.step({a: good_a, 7: good_a})
    with pytest.raises(ValueError, match="seq"):                             # a packet of a later chunk
        pool.step({a: (tp1 + its[0]["pk"][-1:], ap1, None, afp1)}, {b: good_b})
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip((pool.carry, pool.qa_carry, pool.hist), state))
    assert {sid: list(v) for sid, v in pool._sess.items()} == sess and pool.active == (a, b)
    # the sessions go on and still match the solo ones
    out = pool.step({a: good_a}, {b: good_b})
    assert torch.equal(out[a], solo[0].push([tp1], audio_packets=[ap1], audio_fec_packets=[afp1]))
    assert torch.equal(out[b], solo[1].finish([tpb], [apb], tokens=11, audio_fec_packets=[afpb]))
    tp2, ap2, _, afp2 = _chunk_of(its[0], 2, True)
    out = pool.step({}, {a: stream.PoolChunk(tp2, ap2, None, afp2, tokens=5)})
    assert torch.equal(out[a], solo[0].finish([tp2], [ap2], tokens=5, audio_fec_packets=[afp2])) and pool.active == ()
    # the sender pool: a refused tick moves nothing either
    tx = net.stream_sender_pool_av(slots=2, rate=RATE, audio_rate=ARATE, fec=FEC, audio_fec=AFEC)
    ref = net.stream_sender(batch=1, rate=RATE, audio="packets", audio_rate=ARATE, fec=FEC, audio_fec=AFEC)
    s, t_ = its[0]["a"], its[0]["t"]
    u, v = tx.open(), tx.open()
    first = tx.step({u: (s[..., :5120], t_[..., :5120]), v: (s[..., :320], t_[..., :320])})
    want = ref.push(s[..., :5120], t_[..., :5120])
    assert first[u] == first[v] == ([], [], [], []) and want == ([[]], [[]], [[]], [[]])
    with pytest.raises(ValueError, match="StreamSenderPoolAV: session 1.*1 <= m <= 16"):
        tx.step({u: (s[..., 5120:7680], t_[..., 5120:7680]), v: (s[..., :100], t_[..., :100])})
    with pytest.raises(ValueError, match="both pushed and finished"):
        tx.step({u: (s[..., 5120:7680], t_[..., 5120:7680])}, {u: None})
    got = tx.step({u: (s[..., 5120:7680], t_[..., 5120:7680])}, {v: None})
    want = ref.push(s[..., 5120:7680], t_[..., 5120:7680])
    assert all(_same(g, w) for g, w in zip(got[u], want)) and len(got[u][0]) == 8 and len(got[u][2]) == 2 and len(got[u][3]) == 2
    assert got[v][2:4] == (StreamInfo(512, 8, 1, 2), StreamInfo(1024, 32, 1, 2)) and len(got[v]) == 6 and len(got[v][0]) == 1
