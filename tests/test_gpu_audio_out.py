"""-m gpu: the receiver's audio output.  Every comparison is an equality.

  1. mvq_audio_fade_f32 against the numpy definition (tests/audio_out_oracle.py, checked against itself in tests/test_audio_out_cpu.py),
     bit for bit through an integer view: three fades, seven masks, per-item different rows, NaN / 1e30 / -0 payloads;
  2. the same sequences chunk by chunk through the kernel with its state buffer against the whole-item call, the state row against
     the oracle's after every step;
  3. the slot form: guarded rows, a reversed group, an out-of-range slot in a direct C call, an empty group;
  4. the refusals of the C entry points, y and the state untouched;
  5. the whole item: decompress_packets_av(audio_out=True) against ops.audio_fade_ applied by hand to audio_decoder(qa);
  6. streaming: StreamReceiver(audio_out=True) eager and as a graph, both decoder modes, against the whole-item call;
  7. the pool: StreamReceiverPoolAV(audio_out=True) per session against a solo StreamReceiver(batch=1)."""
import numpy as np
import pytest
import torch

import audio_out_oracle as ao
from multimodal_vqvae_compression_audio_tactile_amd import packets, stream
from multimodal_vqvae_compression_audio_tactile_amd.packets import AudioFade, StreamInfo
from test_gpu_av import _channel, _signals
from test_gpu_pool_av import AFEC, FEC, OPENS, TOKENS, _chunk_of, _item
from test_gpu_sender import _net, _stream

pytestmark = pytest.mark.gpu

f32 = np.float32
_REF = {}
GUARD = 0x7FC00000                                       # a NaN's bits: what an untouched int32 state row must still hold
AUDIO_SEEDS = {37: (6, 25), 75: (12, 35), 11: (11, 44)}  # _channel seeds under which an item loses a single token and a longer run
FADE = AudioFade(1, 4)


def _bits(x):
    return np.ascontiguousarray(x, f32).view(np.int32)


def _dbits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def _anet(dev):
    """The shared b8_k512 model with a seeded audio decoder attached: golden_inputs' generator under another seed."""
    net = _net(dev)
    if net.audio_decoder is None:
        import golden_inputs as gi
        from multimodal_vqvae_compression_audio_tactile_amd import DAC
        dec = DAC().decoder
        sd = gi.model_state(23, 8, 512)
        dec.load_state_dict({k[len("T_DEC."):]: v for k, v in sd.items() if k.startswith("T_DEC.")}, strict=True)
        keys = list(net.state_dict().keys())
        net.set_audio_decoder(dec)
        assert list(net.state_dict().keys()) == keys and next(net.audio_decoder.parameters()).device == dev
    return net


def _poisoned(B, T, valid, H, F, seed):
    """A payload with a NaN, 1e30 and -0 at samples of gain 0 and at samples between two gains of 1 -> (y, gain-1 mask, gain-0 mask)."""
    y = ao.payload(B, T, seed)
    _, gain = ao.whole(y, valid, H, F)
    one, zero = gain == 1, gain == 0
    yb = _bits(y).copy()
    for k, word in enumerate((0x7FC12345, 0x7149F2CA, -0x80000000)):
        sel = np.zeros_like(one)
        sel.reshape(-1)[k::3] = True
        yb[zero & sel] = word
        sel.reshape(-1)[:] = False
        sel.reshape(-1)[k::11] = True
        yb[one & sel] = word
    return yb.view(f32), one, zero


# ------------------------------------------------------------------------------------------- 1. the kernel against numpy
@pytest.mark.parametrize("B,T", [(1, 1), (3, 37), (2, 16)])
def test_kernel_equals_numpy_bit_for_bit(B, T, dev):
    from multimodal_vqvae_compression_audio_tactile_amd import ops, torch_ops  # noqa: F401  (registers the operators)
    seen_zero = seen_ramp = False
    for H, F in ao.FADES:
        for name, valid in ao.masks_for(B, T, H, F).items():
            y, one, zero = _poisoned(B, T, valid, H, F, seed=T + 7 * H + F)
            want, gain = ao.whole(y, valid, H, F)
            yd = torch.from_numpy(y.copy()).to(dev).view(B, 1, -1)
            vd = torch.from_numpy(valid).to(dev)
            st = ops.audio_fade_state(B, dev)
            assert ops.audio_fade_(yd, vd, st, AudioFade(H, F), 0) is yd
            got = _dbits(yd).reshape(B, -1)
            assert np.array_equal(got, _bits(want)), (name, H, F)
            assert np.array_equal(got[one], _bits(y)[one]) and not got[zero].any(), (name, H, F)
            r_last = np.stack([np.concatenate([np.zeros(ao.STATE, np.int64), ao.runs(valid[b], H, F)])[-ao.STATE:] for b in range(B)])
            assert np.array_equal(st.cpu().numpy(), r_last), (name, H, F)
            seen_zero |= bool(zero.any())
            seen_ramp |= bool(((gain > 0) & (gain < 1)).any())
            if name == "alternating" and (H, F) == (1, 4):                       # the operator face runs the same launch
                y2, st2 = torch.from_numpy(y.copy()).to(dev).view(B, 1, -1), ops.audio_fade_state(B, dev)
                torch.ops.mi355x_vqvae.audio_fade(y2, vd, st2, H, F, 0)
                assert torch.equal(y2.view(torch.int32), yd.view(torch.int32)) and torch.equal(st2, st)
    assert seen_ramp and (seen_zero or T == 1)                # one token has 312 samples: its ramp never reaches the gain 0 of sample 320


# ------------------------------------------------------------------------------------------------------------ 2. pieces
@pytest.mark.parametrize("B,T", [(1, 1), (1, 11), (2, 16), (3, 37), (2, 75)])
def test_pieces_through_the_state_equal_the_whole_item(B, T, dev):
    from multimodal_vqvae_compression_audio_tactile_amd import ops
    for H, F in ao.FADES:
        for name, valid in ao.masks_for(B, T, H, F).items():
            y, _, _ = _poisoned(B, T, valid, H, F, seed=3 * T + H)
            whole = torch.from_numpy(y.copy()).to(dev).view(B, 1, -1)
            vd = torch.from_numpy(valid).to(dev)
            ops.audio_fade_(whole, vd, ops.audio_fade_state(B, dev), AudioFade(H, F), 0)
            _, states = ao.pieces(y, valid, H, F)
            st = torch.full((B, ao.STATE), GUARD, dtype=torch.int32, device=dev)   # a first step reads no state
            yd, parts = torch.from_numpy(y.copy()).to(dev), []
            for k, (before, n, last) in enumerate(ao.steps(T)):
                tok0, s0, s1 = ao.piece_range(before, n, last)
                if s1 == s0:
                    continue
                part = yd[:, s0:s1].clone().view(B, 1, -1)
                ops.audio_fade_(part, vd[:, before:before + n].contiguous() if n else None, st, AudioFade(H, F), tok0)
                parts.append(part)
                assert np.array_equal(st.cpu().numpy(), states[k]), (name, H, F, k)
            got = torch.cat(parts, dim=-1)
            assert got.shape == whole.shape and torch.equal(got.view(torch.int32), whole.view(torch.int32)), (name, H, F)


# ------------------------------------------------------------------------------------------------------------- 3. slots
def test_slot_form(dev):
    from multimodal_vqvae_compression_audio_tactile_amd import MvqError, _lib, ops
    lib, S, T, (H, F) = _lib.lib(), 4, 37, (1, 4)
    fade = AudioFade(H, F)
    valid = ao.masks_for(2, T, H, F)["border_run"]
    y = ao.payload(2, T, seed=9)
    want, _ = ao.whole(y, valid, H, F)
    _, states = ao.pieces(y, valid, H, F)
    pool = torch.full((S, ao.STATE), GUARD, dtype=torch.int32, device=dev)
    slots = [2, 0]                                                               # item 0 is slot 2, item 1 slot 0
    vd, yd, parts = torch.from_numpy(valid).to(dev), torch.from_numpy(y.copy()).to(dev), []
    for k, (before, n, last) in enumerate(ao.steps(T)):
        tok0, s0, s1 = ao.piece_range(before, n, last)
        part = yd[:, s0:s1].clone().view(2, 1, -1)
        ops.audio_fade_(part, vd[:, before:before + n].contiguous(), pool, fade, tok0, slots=slots)
        parts.append(part)
        got = pool.cpu().numpy()
        assert np.array_equal(got[2], states[k][0]) and np.array_equal(got[0], states[k][1]), k
        assert (got[[1, 3]] == GUARD).all(), k                                   # rows that no slot names stay as they were
    assert np.array_equal(_dbits(torch.cat(parts, dim=-1)).reshape(2, -1), _bits(want))
    # the device copy of the list, when the caller uploaded it already
    p1, p2 = yd[:, :1920].clone().view(2, 1, -1), yd[:, :1920].clone().view(2, 1, -1)
    pa, pb = pool.clone(), pool.clone()
    ops.audio_fade_(p1, vd[:, :16].contiguous(), pa, fade, 0, slots=slots)
    ops.audio_fade_(p2, vd[:, :16].contiguous(), pb, fade, 0, slots=slots, slots_dev=torch.tensor(slots, dtype=torch.int32, device=dev))
    assert torch.equal(p1.view(torch.int32), p2.view(torch.int32)) and torch.equal(pa, pb)
    # an out-of-range slot in a direct C call: it reads "no loss so far" and stores nothing
    before, n = 16, 16
    tok0, s0, s1 = ao.piece_range(before, n, False)
    pool2 = torch.from_numpy(np.stack([states[0][1], np.full(ao.STATE, GUARD), states[0][0], np.full(ao.STATE, GUARD)]).astype(np.int32)).to(dev)
    keep = pool2.clone()
    part = yd[:, s0:s1].clone().view(2, 1, -1)
    sd = torch.tensor([2, 7], dtype=torch.int32, device=dev)
    vchunk = vd[:, before:before + n].contiguous()
    rc = lib.mvq_audio_fade_slots_f32(part.data_ptr(), vchunk.data_ptr(), pool2.data_ptr(), sd.data_ptr(), 2, S, n, tok0, s1 - s0, H, F, _stream())
    assert rc == 0, lib.mvq_last_error()
    got = pool2.cpu().numpy()
    assert np.array_equal(got[2], states[1][0]) and np.array_equal(got[[0, 1, 3]], keep.cpu().numpy()[[0, 1, 3]])
    alone, _ = ao.piece(y[1, s0:s1], valid[1, before:before + n], np.zeros(ao.STATE, np.int64), H, F, before, n, False)
    assert np.array_equal(_dbits(part)[1, 0], _bits(alone)) and np.array_equal(_dbits(part)[0, 0], _bits(want[0, s0:s1]))
    # an empty group launches nothing; the wrapper refuses a bad list on the host
    keep, ykeep = pool2.clone(), part.clone()
    assert lib.mvq_audio_fade_slots_f32(part.data_ptr(), vd.data_ptr(), pool2.data_ptr(), sd.data_ptr(), 0, S, n, tok0, s1 - s0, H, F, _stream()) == 0
    for bad, what in (([0, S], "outside"), ([-1, 0], "outside"), ([1, 1], "twice"), ([0], "1 slots"), (torch.tensor([0, 1]), "host integers")):
        with pytest.raises(MvqError, match=what):
            ops.audio_fade_(part, vd[:, before:before + n].contiguous(), pool2, fade, tok0, slots=bad)
    with pytest.raises(MvqError, match="state"):
        ops.audio_fade_(part, vd[:, before:before + n].contiguous(), pool2.float(), fade, tok0, slots=slots)
    torch.cuda.synchronize()
    assert torch.equal(pool2, keep) and torch.equal(part.view(torch.int32), ykeep.view(torch.int32))


# ---------------------------------------------------------------------------------------------------------- 4. refusals
def test_refusals_leave_everything_untouched(dev):
    from multimodal_vqvae_compression_audio_tactile_amd import MvqError, _lib, ops
    lib = _lib.lib()
    y = torch.from_numpy(ao.payload(2, 7, seed=1)[:, :1920].copy()).to(dev).view(2, 1, 1920)
    v = torch.zeros(2, 16, dtype=torch.uint8, device=dev)
    st = torch.full((4, ao.STATE), 3, dtype=torch.int32, device=dev)
    sd = torch.tensor([0, 1], dtype=torch.int32, device=dev)
    ykeep, skeep = y.clone(), st.clone()
    dense = lambda n, tok0, ln, H, F, yp=y.data_ptr(), vp=v.data_ptr(), sp=st.data_ptr(): \
        lib.mvq_audio_fade_f32(yp, vp, sp, 2, n, tok0, ln, H, F, _stream())
    slots = lambda n, tok0, ln, H, F, yp=y.data_ptr(), vp=v.data_ptr(), sp=st.data_ptr(), lp=sd.data_ptr(), G=2, S=4: \
        lib.mvq_audio_fade_slots_f32(yp, vp, sp, lp, G, S, n, tok0, ln, H, F, _stream())
    for call in (dense, slots):
        for args in ((16, 0, 1920, 1, 0), (16, 0, 1920, -1, 4), (16, 0, 1920, 128, 128), (16, 0, 1919, 1, 4), (16, 0, 1600, 1, 4),
                     (16, 6, 1920, 1, 4), (16, 0, 1920 - 8, 1, 4), (7, 0, 1920 - 8, 1, 4)):   # a finish of 16 / 7 tokens has more samples
            assert call(*args) == -1, args
        assert call(16, 0, 1920, 1, 4, yp=None) == -1 and call(16, 0, 1920, 1, 4, vp=None) == -1 and call(16, 0, 1920, 1, 4, sp=None) == -1
    assert slots(16, 0, 1920, 1, 4, lp=None) == -1 and slots(16, 0, 1920, 1, 4, G=5) == -1
    with pytest.raises(MvqError, match="len"):
        ops.audio_fade_(y[:, :, :1916].contiguous(), v, st[:2].contiguous(), FADE, 0)
    with pytest.raises(MvqError, match="state"):
        ops.audio_fade_(y, v, st.float(), FADE, 0)
    with pytest.raises(MvqError, match="valid"):
        ops.audio_fade_(y, v[:1], st[:2].contiguous(), FADE, 0)
    torch.cuda.synchronize()
    assert torch.equal(y.view(torch.int32), ykeep.view(torch.int32)) and torch.equal(st, skeep)


# -------------------------------------------------------------------------------------------------------- 5. whole item
def _lossy_item(dev, T):
    """B = 2 items of T tokens through compress_packets_av and _channel on both streams -- once per T."""
    if ("lossy", T) not in _REF:
        net = _anet(dev)
        a, t = _signals(dev, 2, 320 * T)
        infos, pk, ainfos, apk = net.compress_packets_av(a, t)
        info, ainfo = infos[0], ainfos[0]
        assert info == StreamInfo(512, 8, T, 2) and ainfo == StreamInfo(1024, 32, T, 2)
        rx = [_channel(pk[b], info, 10 * b + 1)[0] for b in range(2)]
        arx = [_channel(apk[b], ainfo, AUDIO_SEEDS[T][b])[0] for b in range(2)]
        hi, hv, hc, ha = [], [], [], []
        for b in range(2):
            i_b, v_b = packets.unpack_bodies(*packets.gather(rx[b], info), info)
            c_b, a_b = packets.unpack_bodies(*packets.gather(arx[b], ainfo), ainfo)
            hi.append(i_b); hv.append(v_b); hc.append(c_b); ha.append(a_b)
        to = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
        nav = np.stack(ha).astype(np.uint8)
        for b in range(2):                                                    # the channel loses whole audio tokens: a single one, a run
            lens = [len(r) for r in "".join("x" if v == 0 else " " for v in nav[b]).split()]
            assert 1 in lens and max(lens) >= 2, (T, b, lens)
        _REF[("lossy", T)] = dict(info=info, ainfo=ainfo, pk=pk, apk=apk, rx=rx, arx=arx, idx=to(np.stack(hi, axis=1)),
                                  nbv=to(np.stack(hv).astype(np.uint8)), codes=to(np.stack(hc, axis=0)), nav=to(nav), nav_h=nav)
    return _REF[("lossy", T)]


def _whole(dev, T, audio_conceal, fade=FADE):
    key = ("whole", T, audio_conceal, fade)
    if key not in _REF:
        it, net = _lossy_item(dev, T), _anet(dev)
        _REF[key] = net.decompress_packets_av([it["info"]] * 2, it["rx"], [it["ainfo"]] * 2, it["arx"], audio_conceal=audio_conceal,
                                              audio_out=True, audio_fade=fade)
    return _REF[key]


@pytest.mark.parametrize("audio_conceal", ["zero", "mask", "hold"])
def test_whole_item_audio_output(audio_conceal, dev):
    from multimodal_vqvae_compression_audio_tactile_amd import ops
    T = 37
    net, it = _anet(dev), _lossy_item(dev, T)
    y, lost, alost, y_audio = _whole(dev, T, audio_conceal)
    plain = net.decompress_packets_av([it["info"]] * 2, it["rx"], [it["ainfo"]] * 2, it["arx"], audio_conceal=audio_conceal)
    assert len(plain) == 3 and all(torch.equal(g, w) for g, w in zip((y, lost, alost), plain))
    assert torch.equal(alost, it["nav"] == 0) and y_audio.shape == (2, 1, 320 * T - 8)
    z, qa = net.decode_latents(it["codes"], it["idx"], nb_valid=it["nbv"], na_valid=it["nav"], audio_conceal=audio_conceal, return_qa=True)
    assert torch.equal(z, net.decode_latents(it["codes"], it["idx"], nb_valid=it["nbv"], na_valid=it["nav"], audio_conceal=audio_conceal))
    lost_cols = qa.permute(0, 2, 1)[alost]                                     # [lost tokens, C]
    if audio_conceal == "hold":                                               # the held token (the first loss of item 0 follows an arrival)
        b, t = [int(v) for v in torch.nonzero(alost)[0]]
        first_ok = t > 0 and not bool(alost[b, t - 1])
        assert not first_ok or torch.equal(qa[b, :, t], qa[b, :, t - 1])
        assert bool(lost_cols.any())
    else:                                                                     # +0 at a lost token: from_codes writes it, "mask" leaves it
        assert not bool(lost_cols.view(torch.int32).any())
    by_hand = net.audio_decoder(qa).contiguous()
    raw = by_hand.clone()
    ops.audio_fade_(by_hand, it["nav"], ops.audio_fade_state(2, dev), FADE, 0)
    assert torch.equal(y_audio, by_hand) and not torch.equal(y_audio, raw)
    want, _ = ao.whole(raw.cpu().numpy().reshape(2, -1), it["nav_h"], FADE.hold_tok, FADE.fade_tok)
    assert np.array_equal(_dbits(y_audio).reshape(2, -1), _bits(want))
    assert torch.equal(_whole(dev, T, audio_conceal, None)[3], raw)           # audio_fade=None skips the kernel
    ya2 = net.decode_av(it["codes"], it["idx"], nb_valid=it["nbv"], na_valid=it["nav"], audio_conceal=audio_conceal, audio_fade=FADE)
    assert torch.equal(ya2[0], y) and torch.equal(ya2[1], y_audio)
    print(f"audio out {audio_conceal}: lost tokens {int(alost.sum())}, sum|y_audio| {float(y_audio.abs().sum()):.6g} raw {float(raw.abs().sum()):.6g} "
          f"finite={bool(torch.isfinite(y_audio).all())} device={torch.cuda.get_device_name(dev)}")


def test_whole_item_without_loss_is_the_plain_decode(dev):
    net, it = _anet(dev), _lossy_item(dev, 37)
    a, t = _signals(dev, 2, 320 * 37)
    _, codes, _ = net.encode_latents_with_indices(a, t)
    want = net.audio_decoder(net.A_QUANT.from_codes(codes)[0])
    ref = net.decompress_packets_av([it["info"]] * 2, it["pk"], [it["ainfo"]] * 2, it["apk"])
    for fade in (None, AudioFade(0, 1), FADE, AudioFade(2, 3)):
        y, lost, alost, y_audio = net.decompress_packets_av([it["info"]] * 2, it["pk"], [it["ainfo"]] * 2, it["apk"], audio_out=True,
                                                            audio_fade=fade)
        assert torch.equal(y_audio, want) and torch.equal(y, ref[0]) and not bool(alost.any()) and not bool(lost.any())


# --------------------------------------------------------------------------------------------------------- 6. streaming
def _seq(p):
    return int.from_bytes(bytes(p)[3:7], "little")


STREAM_CASES = [(75, g, d, c) for g in (False, True) for d in ("window", "stateful") for c in ("zero", "hold")] + \
               [(T, False, d, c) for T in (37, 11) for d in ("window", "stateful") for c in ("zero", "hold")]


@pytest.mark.parametrize("T,graph,decoder,audio_conceal", STREAM_CASES)
def test_stream_receiver_audio_output_equals_the_whole_item(T, graph, decoder, audio_conceal, dev):
    net, it = _anet(dev), _lossy_item(dev, T)
    want_y, _, alost, want_a = _whole(dev, T, audio_conceal)
    rx = net.stream_receiver(512, 8, batch=2, graph=graph, audio=(1024, 32), audio_conceal=audio_conceal, decoder=decoder, audio_out=True,
                             audio_fade=FADE)
    ys, yas = [], []
    for c in range(T // 16):
        pick = lambda lists: [[p for p in lists[b] if 8 * c <= _seq(p) < 8 * c + 8] for b in range(2)]
        y, ya = rx.push(pick(it["rx"]), audio_packets=pick(it["arx"]))
        assert y.shape == ya.shape
        ys.append(y.clone()); yas.append(ya.clone())
    tail = lambda lists: [[p for p in lists[b] if _seq(p) >= 8 * (T // 16)] for b in range(2)]
    y, ya = rx.finish(tail(it["rx"]), tail(it["arx"]), tokens=T % 16)
    ys.append(y); yas.append(ya)
    got_y, got_a = torch.cat(ys, dim=-1), torch.cat(yas, dim=-1)
    assert got_y.shape == want_y.shape and torch.equal(got_y, want_y)
    assert got_a.shape == want_a.shape and torch.equal(got_a.view(torch.int32), want_a.view(torch.int32))
    if T == 11:
        assert len(ys) == 1                                                   # the finish-only path
    if graph:                                                                 # captured at chunk 2, replayed at chunk 3 under another pattern
        assert rx._g is not None and isinstance(rx._g[0], torch.cuda.CUDAGraph) and len(rx._g[3]) == 2
        assert not torch.equal(alost[:, 32:48], alost[:, 48:64]) and bool(alost[:, 48:64].any())


# -------------------------------------------------------------------------------------------------------------- 7. pool
def _parts(it, c, last, fec):
    tp, ap, fp, afp = _chunk_of(it, c, last)
    return (tp, ap, fp, afp) if fec else (tp, ap)


def _solo_av(dev, i, kw, fec):
    it, T = _item(dev, i), TOKENS[i]
    rx = _anet(dev).stream_receiver(512, 8, batch=1, audio=(1024, 32), **kw)
    outs = []
    for c in range(T // 16):
        p = _parts(it, c, False, fec)
        outs.append(tuple(o.clone() for o in rx.push([p[0]], audio_packets=[p[1]], **(dict(fec_packets=[p[2]], audio_fec_packets=[p[3]]) if fec else {}))))
    if T % 16:
        p = _parts(it, T // 16, True, fec)
        outs.append(rx.finish([p[0]], [p[1]], tokens=T % 16, **(dict(fec_packets=[p[2]], audio_fec_packets=[p[3]]) if fec else {})))
    else:
        outs.append(rx.finish())
    return outs


@pytest.mark.parametrize("decoder,audio_conceal,fec", [("window", "zero", False), ("stateful", "hold", True)])
def test_pool_av_audio_output_equals_the_solo_receiver(decoder, audio_conceal, fec, dev):
    net = _anet(dev)
    kw = dict(audio_conceal=audio_conceal, decoder=decoder, audio_out=True, audio_fade=FADE)
    if fec:
        kw.update(fec=FEC, audio_fec=AFEC)
        assert any(_item(dev, i)["arule"][0] for i in range(len(TOKENS)))      # an audio token comes back from the parity: not faded
    pool = stream.StreamReceiverPoolAV(net, 512, 8, slots=4, audio=(1024, 32), **kw)
    pool.fade_state.fill_(GUARD)                                              # open() clears nothing: a new session reads no run length
    for state in (pool.a_hist, pool.a_dec_state):
        if state is not None:
            state.fill_(float("nan"))
    sids, nxt, done, outs, tick = {}, {}, set(), {k: [] for k in range(len(TOKENS))}, 0
    while len(done) < len(TOKENS):
        for k, t0 in enumerate(OPENS):
            if t0 == tick:
                sids[k], nxt[k] = pool.open(), 0
        pushes, finishes = {}, {}
        for k, sid in sids.items():
            if k in done:
                continue
            it, T, c = _item(dev, k), TOKENS[k], nxt[k]
            if 16 * (c + 1) <= T:
                pushes[sid] = _parts(it, c, False, fec)
            elif T % 16:
                finishes[sid] = stream.PoolChunk(*_parts(it, c, True, fec), tokens=T % 16)
            else:
                finishes[sid] = None
        out = pool.step(pushes, finishes)
        for k, sid in sids.items():
            if sid in out:
                outs[k].append(out[sid])
            if sid in pushes:
                nxt[k] += 1
            elif sid in finishes:
                done.add(k)
        tick += 1
    assert pool.active == () and pool.free == 4
    faded = False
    for i, T in enumerate(TOKENS):
        solo = _solo_av(dev, i, kw, fec)
        assert len(outs[i]) == len(solo)
        for j, (got, want) in enumerate(zip(outs[i], solo)):                  # call by call, both outputs
            assert isinstance(got, tuple) and len(got) == 2
            assert got[0].shape == want[0].shape and torch.equal(got[0], want[0]), (i, j)
            assert got[1].shape == want[1].shape and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32)), (i, j)
        ya = torch.cat([o[1] for o in outs[i]], dim=-1)
        assert ya.shape == (1, 1, 320 * T - 8) and bool(torch.isfinite(ya).all())
        it = _item(dev, i)
        whole = net.decompress_packets_av([it["info"]], [it["rx"]], [it["ainfo"]], [it["arx"]], audio_conceal=audio_conceal, audio_out=True,
                                          audio_fade=FADE, **(dict(fec=FEC, fec_packets=[it["rxp"]], audio_fec=AFEC,
                                                                   audio_fec_packets=[it["arxp"]]) if fec else {}))
        assert torch.equal(ya.view(torch.int32), whole[3].view(torch.int32)), i
        assert torch.equal(torch.cat([o[0] for o in outs[i]], dim=-1), whole[0]), i
        faded |= bool(whole[2].any())
    assert faded
