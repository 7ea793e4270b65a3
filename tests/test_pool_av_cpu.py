"""No GPU: the pools for the whole link -- the new factories' signatures and the untouched old ones, every
construction refusal of the solo classes under the new class names, ``stream.receiver_layout`` against the bytes
``StreamReceiver(batch=1)._gather`` and the pool's per-session gathering build (restated here from packets.gather / gather_fec),
``_SenderCore._frame_one`` against ``StreamSender._framed`` and against packets.frame / frame_fec, and the argument checks of
mvq_hold_fill_slots_f32.  Every comparison is an equality."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from multimodal_vqvae_compression_audio_tactile_amd import packets, stream
from multimodal_vqvae_compression_audio_tactile_amd.packets import Fec, Rate, StreamInfo

FEC, AFEC = Fec(4, 3), Fec(8, 4, 2)
K, NB, KA, NA, PTOK = 512, 8, 1024, 32, 2


@pytest.fixture(scope="module")
def cpu_net():
    from multimodal_vqvae_compression_audio_tactile_amd import build_proposed
    return build_proposed(None, rvq_books=NB, rvq_embed=K, device="cpu")


# ---------------------------------------------------------------------------------------------------------- 1. the surface
def _sig(fn):
    return [(n, p.default) for n, p in inspect.signature(fn).parameters.items() if n != "self"]


def test_factory_signatures():
    from multimodal_vqvae_compression_audio_tactile_amd import ProposedEval
    E = inspect.Parameter.empty
    assert _sig(ProposedEval.stream_sender_pool_av) == [
        ("packet_tok", 2), ("slots", 64), ("books_use", None), ("rate", None), ("audio", "packets"), ("audio_books", None),
        ("audio_rate", None), ("fec", None), ("audio_fec", None), ("encoder", "window")]
    assert _sig(ProposedEval.stream_receiver_pool_av) == [
        ("K", E), ("nb", E), ("packet_tok", 2), ("slots", 64), ("books_use", None), ("conceal", "predict"), ("out_rate", 24000),
        ("audio", None), ("fec", None), ("audio_fec", None), ("audio_conceal", "zero"), ("decoder", "window")]
    # the existing factories are what they were
    assert _sig(ProposedEval.stream_sender_pool) == [("packet_tok", 2), ("slots", 64), ("books_use", None), ("encoder", "window")]
    assert _sig(ProposedEval.stream_receiver_pool) == [
        ("K", E), ("nb", E), ("packet_tok", 2), ("slots", 64), ("books_use", None), ("conceal", "predict"), ("out_rate", 24000),
        ("audio_conceal", None), ("decoder", "window")]
    assert issubclass(stream.StreamSenderPoolAV, stream.StreamSenderPool) and issubclass(stream.StreamReceiverPoolAV, stream.StreamReceiverPool)
    for cls, base in ((stream.StreamSenderPoolAV, stream.StreamSenderPool), (stream.StreamReceiverPoolAV, stream.StreamReceiverPool)):
        for name in ("open", "close", "active", "free", "tokens", "_get"):          # session management is shared, not copied
            assert getattr(cls, name) is getattr(base, name), (cls, name)
    assert stream.StreamReceiverPoolAV.late is stream.StreamReceiverPool.late
    assert stream.StreamSenderPoolAV._inputs is stream.StreamSenderPool._inputs and stream.StreamSenderPoolAV.step is stream.StreamSenderPool.step
    assert stream.PoolChunk._fields == ("tactile_packets", "audio", "fec_packets", "audio_fec_packets", "tokens")
    assert stream.PoolChunk([], [])[2:] == (None, None, None)


def _message(call, exc=ValueError):
    with pytest.raises(exc) as e:
        call()
    return str(e.value)


SENDER_REFUSALS = [dict(packet_tok=3), dict(encoder="ring"), dict(audio="both"), dict(audio="codes", audio_books=4),
                   dict(audio="codes", audio_rate=Rate()), dict(audio="codes", audio_fec=AFEC), dict(audio="packets", audio_books=33),
                   dict(audio="packets", audio_books=4, audio_rate=Rate(min_books=5)), dict(rate=Rate(min_books=9)), dict(fec="xor"),
                   dict(fec=Fec(3, 3)), dict(fec=Fec(4, 9)), dict(fec=Fec(4, 3, 5)), dict(audio="packets", audio_fec=Fec(8, 33)),
                   dict(audio="packets", audio_fec=Fec(16, 4)), dict(packet_tok=0)]
RECEIVER_REFUSALS = [dict(conceal="plc"), dict(conceal="repeat"), dict(packet_tok=3), dict(out_rate=8000), dict(decoder="ring"),
                     dict(audio_conceal="repeat"), dict(audio_conceal="mask"), dict(audio_conceal="hold"), dict(audio_fec=AFEC),
                     dict(audio=(1024, 33)), dict(audio=(512, 32)), dict(audio=(1024, 32), audio_fec=Fec(8, 33)), dict(fec="xor"),
                     dict(fec=Fec(3, 3)), dict(fec=Fec(4, 9)), dict(fec=Fec(4, 3, 0)), dict(audio=(1024, 32), audio_fec=Fec(16, 4))]


@pytest.mark.parametrize("kw", SENDER_REFUSALS, ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_sender_pool_av_refuses_what_the_solo_sender_refuses(kw, cpu_net):
    solo = _message(lambda: cpu_net.stream_sender(**kw))
    assert _message(lambda: cpu_net.stream_sender_pool_av(**kw)) == solo.replace("StreamSender", "StreamSenderPoolAV")


@pytest.mark.parametrize("kw", RECEIVER_REFUSALS, ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_receiver_pool_av_refuses_what_the_solo_receiver_refuses(kw, cpu_net):
    solo = _message(lambda: cpu_net.stream_receiver(K, NB, **kw))
    assert _message(lambda: cpu_net.stream_receiver_pool_av(K, NB, **kw)) == solo.replace("StreamReceiver", "StreamReceiverPoolAV")


def test_the_remaining_refusals_and_the_allowed_tactile_only_pools(cpu_net):
    from multimodal_vqvae_compression_audio_tactile_amd import MvqError, ops
    assert "slots must be at least 1" in _message(lambda: cpu_net.stream_sender_pool_av(slots=0))
    assert "slots must be at least 1" in _message(lambda: cpu_net.stream_receiver_pool_av(K, NB, slots=0))
    for bad in ((128, NB), (K, 9)):
        solo = _message(lambda: cpu_net.stream_receiver(*bad))
        assert _message(lambda: cpu_net.stream_receiver_pool_av(*bad)) == solo.replace("StreamReceiver", "StreamReceiverPoolAV")
    with ops.arith("f16x3"):
        assert "StreamSenderPoolAV: arithmetic" in _message(lambda: cpu_net.stream_sender_pool_av())
        assert "StreamReceiverPoolAV: arithmetic" in _message(lambda: cpu_net.stream_receiver_pool_av(K, NB))
    # audio="codes" / audio=None are allowed: a tactile-only stream with rate= / fec= gets a pool too
    tx = cpu_net.stream_sender_pool_av(slots=2, audio="codes", rate=Rate(min_books=2, tol2=0.84), fec=FEC)
    assert not tx.audio_packets and tx.fec is FEC and tx.slots == 2 and tx.free == 2 and tx.active == ()
    rx = cpu_net.stream_receiver_pool_av(K, NB, slots=3, fec=FEC)
    assert rx.audio is None and rx.fec is FEC and rx.qa_carry is None and rx.free == 3
    hold = cpu_net.stream_receiver_pool_av(K, NB, slots=3, audio=(KA, NA), audio_fec=AFEC, audio_conceal="hold")
    assert hold.qa_carry.shape == (3, hold.C) and hold.carry.shape == (3, hold.C)
    # open() resets the slot's held audio token beside the carried one
    hold.qa_carry.fill_(float("nan")), hold.carry.fill_(float("nan"))
    sid = hold.open()
    assert sid == 0 and not hold.qa_carry[0].any() and not hold.carry[0].any() and bool(torch.isnan(hold.qa_carry[1:]).all())
    with pytest.raises(MvqError, match="StreamReceiverPoolAV: tokens: no open session 5"):
        hold.tokens(5)
    with pytest.raises(MvqError, match="StreamSenderPoolAV: close: no open session 0"):
        tx.close(0)
    # a tick's refusals come before anything moves
    codes = torch.zeros(32, 16, dtype=torch.int64)
    with pytest.raises(ValueError, match="StreamReceiverPoolAV: session 0: fec_packets / audio_fec_packets need a pool opened with"):
        hold.step({sid: ([], [], [])})
    with pytest.raises(ValueError, match="tokens = None"):
        hold.step({}, {sid: ([], [])})
    with pytest.raises(ValueError, match="tokens = 16"):
        hold.step({}, {sid: stream.PoolChunk([], [], tokens=16)})
    with pytest.raises(ValueError, match="belongs to a finish"):
        hold.step({sid: stream.PoolChunk([], [], tokens=5)})
    with pytest.raises(ValueError, match="both pushed and finished"):
        hold.step({sid: ([], [])}, {sid: None})
    with pytest.raises(ValueError, match="a push needs"):
        hold.step({sid: None})
    with pytest.raises(ValueError, match="expected"):
        hold.step({sid: ([],)})
    s2 = rx.open()
    with pytest.raises(ValueError, match="audio_fec_packets need a pool opened with"):
        rx.step({s2: ([], codes, None, [])})
    with pytest.raises(ValueError, match="audio codes carry their own length"):
        rx.step({}, {s2: stream.PoolChunk([], codes[:, :5], tokens=5)})
    with pytest.raises(ValueError, match="StreamReceiverPoolAV: session 0: 17 audio tokens"):
        rx.step({s2: ([], torch.zeros(32, 17, dtype=torch.int64))})
    assert hold.tokens(sid) == 0 and hold.late(sid) == 0 and rx.tokens(s2) == 0 and hold.active == (sid,)


# ------------------------------------------------------------------------------------------------------------ 2. the layout
def _chunk(rng, n, chunk):
    """One chunk of ``n`` tokens as chunk ``chunk`` of a stream sends it: (info, ainfo, packets, audio packets, parity, audio parity)."""
    info, ainfo = StreamInfo(K, NB, n, PTOK), StreamInfo(KA, NA, n, PTOK)
    out = []
    for inf, f in ((info, FEC), (ainfo, AFEC)):
        bodies = packets.pack_bodies(rng.integers(0, inf.K, size=(inf.nb, n)), inf)
        sent = rng.integers(1, inf.nb + 1, size=inf.P)
        base = chunk * 16 // PTOK
        out.append((packets.frame(bodies, inf, nb_sent=sent, seq_base=base),
                    packets.frame_fec(packets.fec_rows(bodies, sent, inf, f), inf, f, seq_base=base // f.group)))
    return info, ainfo, out[0][0], out[1][0], out[0][1], out[1][1]


@pytest.mark.parametrize("parity", ["present", "lost", "absent"])
@pytest.mark.parametrize("n", [16, 11])
def test_receiver_layout_is_what_gather_builds(n, parity, cpu_net):
    rng = np.random.default_rng(100 * n + len(parity))
    chunk = 2
    info, ainfo, pk, apk, par, apar = _chunk(rng, n, chunk)
    base = chunk * 16 // PTOK
    rx_pk = [p for i, p in enumerate(pk) if i not in (1, 4)][::-1] + [pk[0]]          # two lost, reordered, one duplicated
    rx_apk = [p for i, p in enumerate(apk) if i != 0]
    if parity == "present":
        rx_par, rx_apar = par[::-1], apar
    elif parity == "lost":                                                   # a group's parity / one of a group's two parity packets
        rx_par, rx_apar = par[1:], apar[1:]
    else:
        rx_par = rx_apar = None
    # restated: the arrays in the order of the layout, each from packets.gather / gather_fec
    parts = [*packets.gather(rx_pk, info, seq_base=base), *packets.gather(rx_apk, ainfo, seq_base=base),
             *packets.gather_fec(rx_par or [], info, FEC, seq_base=base // 4), *packets.gather_fec(rx_apar or [], ainfo, AFEC, seq_base=base // 8)]
    want = np.concatenate([np.asarray(p, np.uint8).reshape(-1) for p in parts])
    sizes = [p.size for p in parts]
    full, afull = packets.body_bytes(PTOK, NB, K), packets.body_bytes(PTOK, NA, KA)
    code = lambda f, inf: (f.resolve(inf)[0], f.r, f.resolve(inf)[3])
    lay = stream.receiver_layout(1, n, full, afull, code(FEC, info), code(AFEC, ainfo), PTOK)
    at = np.cumsum([0] + sizes)
    assert (lay.P, lay.bodies, lay.counts, lay.abodies, lay.acounts) == (info.P, at[0], at[1], at[2], at[3])
    assert lay.fec == (at[4], at[5]) and lay.audio_fec == (at[6], at[7]) and lay.size == at[8] == want.size
    # the lockstep receiver at batch 1
    rx = cpu_net.stream_receiver(K, NB, batch=1, audio=(KA, NA), fec=FEC, audio_fec=AFEC)
    rx.tokens, rx.h = 16 * chunk, 20
    wrap = lambda x: None if x is None else [x]
    host = rx._gather([rx_pk], n, [rx_apk], wrap(rx_par), wrap(rx_apar))
    assert host.dtype == np.uint8 and np.array_equal(host, want) and rx.late == 0
    assert rx._layout(1, n) == lay
    # the pool's per-session gathering: the same arrays in the same order
    pool = cpu_net.stream_receiver_pool_av(K, NB, slots=2, audio=(KA, NA), fec=FEC, audio_fec=AFEC)
    sid = pool.open()
    pool._sess[sid][1] = 16 * chunk
    item = stream.PoolChunk(rx_pk + pk[:0], rx_apk, rx_par, rx_apar, None if n == 16 else n)
    work = pool._inputs({sid: item}, {}) if n == 16 else pool._inputs({}, {sid: item})
    got_n, last, got_parts, codes, late = work[sid]
    assert (got_n, last, codes, late) == (n, n != 16, None, 0)
    assert np.array_equal(np.concatenate([np.asarray(p, np.uint8).reshape(-1) for p in got_parts]), want)
    # G items: every part is G times as long, in the same order
    lay3 = stream.receiver_layout(3, n, full, afull, code(FEC, info), code(AFEC, ainfo), PTOK)
    assert lay3.size == 3 * lay.size and lay3.counts == 3 * lay.counts and lay3.fec == (3 * at[4], 3 * at[4] + 3 * sizes[4])
    # without audio packets / without a Fec the parts are absent
    plain = stream.receiver_layout(2, n, full, None, None, None, PTOK)
    assert plain == stream.RxLayout(info.P, 0, 2 * info.P * full, None, None, None, None, 2 * info.P * (full + 1))


def test_a_late_packet_is_counted_for_its_session(cpu_net):
    rng = np.random.default_rng(3)
    _, _, pk0, apk0, par0, apar0 = _chunk(rng, 16, 0)
    _, _, pk2, apk2, par2, apar2 = _chunk(rng, 16, 2)
    pool = cpu_net.stream_receiver_pool_av(K, NB, slots=2, audio=(KA, NA), fec=FEC, audio_fec=AFEC)
    a, b = pool.open(), pool.open()
    pool._sess[a][1] = pool._sess[b][1] = 32
    work = pool._inputs({a: (pk2 + pk0[:2], apk2 + apk0[:1], par2 + par0[:1], apar2 + apar0[:2]), b: (pk2, apk2)}, {})
    assert work[a][4] == 6 and work[b][4] == 0
    with pytest.raises(ValueError, match="seq"):                             # a packet of a later chunk
        pool._inputs({a: (pk2, apk2)}, {b: stream.PoolChunk(_chunk(rng, 16, 4)[2], apk2, tokens=3)})


# ----------------------------------------------------------------------------------------------------------- 3. the framing
@pytest.mark.parametrize("chunk", [0, 2])
@pytest.mark.parametrize("n_tok", [16, 11])
def test_frame_one_is_what_framed_returns(n_tok, chunk, cpu_net):
    rng = np.random.default_rng(10 * n_tok + chunk)
    info, ainfo = StreamInfo(K, NB, n_tok, PTOK), StreamInfo(KA, NA, n_tok, PTOK)
    base = chunk * 16 // PTOK
    bodies = packets.pack_bodies(rng.integers(0, K, size=(NB, n_tok)), info)
    abodies = packets.pack_bodies(rng.integers(0, KA, size=(NA, n_tok)), ainfo)
    sent, asent = rng.integers(1, NB + 1, size=info.P).astype(np.uint8), rng.integers(1, NA + 1, size=ainfo.P).astype(np.uint8)
    flat = lambda *xs: np.concatenate([np.asarray(x, np.uint8).reshape(-1) for x in xs])
    codes = torch.zeros(1, 32, n_tok, dtype=torch.int64)
    cases = [
        (dict(rate=Rate(min_books=2, tol2=0.84), audio="packets", fec=FEC, audio_fec=AFEC),
         flat(bodies, sent, abodies, asent, packets.fec_rows(bodies, sent, info, FEC), packets.fec_rows(abodies, asent, ainfo, AFEC)),
         (packets.frame(bodies, info, nb_sent=sent, seq_base=base), packets.frame(abodies, ainfo, nb_sent=asent, seq_base=base),
          packets.frame_fec(packets.fec_rows(bodies, sent, info, FEC), info, FEC, seq_base=base // 4),
          packets.frame_fec(packets.fec_rows(abodies, asent, ainfo, AFEC), ainfo, AFEC, seq_base=base // 8))),
        (dict(audio="packets", audio_fec=AFEC),
         flat(bodies, sent, abodies, asent, packets.fec_rows(abodies, asent, ainfo, AFEC)),
         (packets.frame(bodies, info, nb_sent=sent, seq_base=base), packets.frame(abodies, ainfo, nb_sent=asent, seq_base=base), [],
          packets.frame_fec(packets.fec_rows(abodies, asent, ainfo, AFEC), ainfo, AFEC, seq_base=base // 8))),
        (dict(audio="packets"), flat(bodies, sent, abodies, asent),
         (packets.frame(bodies, info, nb_sent=sent, seq_base=base), packets.frame(abodies, ainfo, nb_sent=asent, seq_base=base))),
        (dict(rate=Rate(min_books=2, tol2=0.84), audio="codes", fec=FEC), flat(bodies, sent, packets.fec_rows(bodies, sent, info, FEC)),
         (packets.frame(bodies, info, nb_sent=sent, seq_base=base),
          packets.frame_fec(packets.fec_rows(bodies, sent, info, FEC), info, FEC, seq_base=base // 4))),
        (dict(audio="codes", fec=AFEC.__class__(8, 3, 2)), flat(bodies, packets.fec_rows(bodies, None, info, Fec(8, 3, 2))),
         (packets.frame(bodies, info, seq_base=base), packets.frame_fec(packets.fec_rows(bodies, None, info, Fec(8, 3, 2)), info, Fec(8, 3, 2), seq_base=base // 8))),
        (dict(rate=Rate(budget=27), audio="codes"), flat(bodies, sent), (packets.frame(bodies, info, nb_sent=sent, seq_base=base),)),
        (dict(audio="codes"), flat(bodies), (packets.frame(bodies, info, seq_base=base),)),
    ]
    for kw, row, want in cases:
        tx = cpu_net.stream_sender(batch=1, **kw)
        tx.chunk = chunk
        one = tx._frame_one(row, n_tok, chunk)
        assert one == want, kw
        framed = tx._framed(torch.from_numpy(row.copy())[None], codes, n_tok)
        if kw["audio"] == "packets":
            assert framed == tuple([x] for x in want), kw
        else:
            assert framed[1] is codes and (framed[0],) + framed[2:] == tuple([x] for x in want), kw
        pool = cpu_net.stream_sender_pool_av(slots=2, **kw)
        got = pool._frame(row, n_tok, chunk, codes)
        assert got == (want if kw["audio"] == "packets" else (want[0], codes) + want[1:]), kw
        assert len(pool._nothing()) == len(got) and all(x == [] for x in pool._nothing() if isinstance(x, list))
    # two items of a lockstep sender: each its own row
    tx = cpu_net.stream_sender(batch=2, audio="codes")
    tx.chunk = chunk
    other = packets.pack_bodies(rng.integers(0, K, size=(NB, n_tok)), info)
    pk, _ = tx._framed(torch.from_numpy(np.stack([bodies, other])), None, n_tok)
    assert pk == [packets.frame(bodies, info, seq_base=base), packets.frame(other, info, seq_base=base)]


# ------------------------------------------------------------------------------------------------------------ 4. the export
def test_hold_fill_slots_entry_point_refuses_before_any_launch():
    from multimodal_vqvae_compression_audio_tactile_amd import MvqError, _lib, ops
    assert {"slots", "slots_dev"} <= set(inspect.signature(ops.hold_fill_).parameters)
    from multimodal_vqvae_compression_audio_tactile_amd import ProposedEval
    assert {"qa_slots", "qa_slots_dev"} <= set(inspect.signature(ProposedEval.decode_latents).parameters)
    lib = _lib.lib()
    assert "mvq_hold_fill_slots_f32" in _lib.EXPORTS and hasattr(lib, "mvq_hold_fill_slots_f32")
    assert lib.mvq_abi_version() == 3
    f = lib.mvq_hold_fill_slots_f32
    fake = ctypes.c_void_p(4096)                             # never dereferenced: every call below returns before any launch
    for shape in ((-1, 5, 4, 4), (2, -1, 4, 4), (2, 5, -4, 4), (2, 5, 4, -4), (2, 5, 16 * 65535 + 1, 4)):
        assert f(fake, fake, fake, fake, *shape, None) == -1, shape
    assert f(fake, fake, fake, fake, 2, 5, 16 * 65535 + 1, 4, None) == -1 and b"bad shape" in lib.mvq_last_error()
    assert f(fake, fake, fake, fake, 6, 5, 4, 4, None) == -1 and b"a group of 6 sessions in a pool of 5 slots" in lib.mvq_last_error()
    for args in ((None, fake, fake, fake), (fake, None, fake, fake), (fake, fake, None, fake), (fake, fake, fake, None)):
        assert f(*args, 2, 5, 4, 4, None) == -1 and b"null tensor" in lib.mvq_last_error()
    assert f(None, None, None, None, 0, 5, 4, 4, None) == 0                  # an empty group, no channels, no tokens: no launch
    assert f(None, None, None, None, 2, 5, 0, 4, None) == 0 and f(None, None, None, None, 2, 5, 4, 0, None) == 0
    with pytest.raises(MvqError, match="hold_fill_"):                        # host tensors are refused, slots or not
        ops.hold_fill_(torch.zeros(2, 4, 5), torch.zeros(2, 5, dtype=torch.uint8), torch.zeros(3, 4), slots=[0, 1])
    carry = torch.zeros(2, 1024)
    net_kw = dict(na_valid=torch.full((2, 20), 32, dtype=torch.uint8), audio_conceal="hold")
    from multimodal_vqvae_compression_audio_tactile_amd import build_proposed
    net = build_proposed(None, rvq_books=2, rvq_embed=128, device="cpu")
    idx, codes = torch.zeros(2, 2, 20, dtype=torch.int64), torch.zeros(2, 32, 20, dtype=torch.int64)
    with pytest.raises(MvqError, match="ONE pool buffer"):
        net.decode_latents(codes, idx, qa_prev=carry, qa_slots=[0, 1], **net_kw)
    with pytest.raises(MvqError, match="ONE pool buffer"):
        net.decode_latents(codes, idx, qa_prev=carry, qa_last_out=carry.clone(), qa_slots=[0, 1], **net_kw)
    with pytest.raises(MvqError, match="ONE pool buffer"):
        net.decode_latents(codes, idx, qa_prev=carry, qa_last_out=carry, qa_slots_dev=torch.zeros(2, dtype=torch.int32), **net_kw)
