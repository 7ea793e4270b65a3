"""No GPU: the receiver front end (``stream._RxFront``), the one owner of the upload's format.

  1. layout: ``layout`` + ``gather_item`` + ``fill`` against an independent restatement -- the plain ``np.concatenate`` of
     packets.gather / gather_fec outputs in the documented order (tactile bodies, counts, audio bodies, counts, then per stream with
     a Fec its parity rows and ``got`` flags), item 0..G-1 within each part -- and ``StreamReceiver._gather`` against the same bytes;
  2. pool upload: the host array of a plain-pool tick with two groups against the arithmetic the pool used before it went through
     the front end, restated here: the slot lists, then per group the bodies [G, P, full] and the counts [G, P].

Every comparison is an equality."""
import numpy as np
import pytest
import torch

from multimodal_vqvae_compression_audio_tactile_amd import packets, stream
from multimodal_vqvae_compression_audio_tactile_amd.packets import Fec, StreamInfo

K, NB, KA, NA, PTOK = 512, 8, 1024, 32, 2
OPTIONS = {"tactile": {}, "audio": dict(audio=(KA, NA)), "fec1": dict(fec=Fec(4, 3)),
           "fec2+afec": dict(audio=(KA, NA), fec=Fec(4, 3, 2), audio_fec=Fec(8, 4, 2))}


@pytest.fixture(scope="module")
def cpu_net():
    from multimodal_vqvae_compression_audio_tactile_amd import build_proposed
    return build_proposed(None, rvq_books=NB, rvq_embed=K, device="cpu")


def _sent(rng, info, fec, seq_base):
    """One item's stream as the sender numbers it from packet ``seq_base`` on -> (packets, parity packets or None)."""
    bodies = packets.pack_bodies(rng.integers(0, info.K, size=(info.nb, info.T)), info)
    sent = rng.integers(1, info.nb + 1, size=info.P)
    par = None if fec is None else packets.frame_fec(packets.fec_rows(bodies, sent, info, fec), info, fec, seq_base=seq_base // fec.group)
    return packets.frame(bodies, info, nb_sent=sent, seq_base=seq_base), par


def _arrived(pk, i, stale):
    """What arrives of ``pk``: packet i % P is missing, the next one comes twice, and (``stale`` not None) one of an earlier chunk."""
    P = len(pk)
    return [p for s, p in enumerate(pk) if s != i % P][::-1] + [pk[(i + 1) % P]] + ([] if stale is None else [stale])


def _items(opt, G, n, seq_base, seed):
    """G items' arrived packets per list (tactile, audio, parity, audio parity; None where the options have no such list) and the
    stale packets among them."""
    rng = np.random.default_rng(seed)
    streams = [(StreamInfo(K, NB, n, PTOK), opt.get("fec"))] + ([(StreamInfo(*opt["audio"], n, PTOK), opt.get("audio_fec"))] if "audio" in opt else [])
    lists, n_late = [[None] * G for _ in range(4)], 0
    for s, (info, fec) in enumerate(streams):
        # an earlier chunk's packets, for the one late packet: 16 tokens before seq_base
        old_pk, old_par = _sent(rng, StreamInfo(info.K, info.nb, 16, PTOK), fec, seq_base - 8) if seq_base else (None, None)
        for i in range(G):
            pk, par = _sent(rng, info, fec, seq_base)
            lists[s][i] = _arrived(pk, i + s, None if old_pk is None else old_pk[i])
            n_late += old_pk is not None
            if par is not None:
                lists[2 + s][i] = par[1:] + ([] if old_par is None else [old_par[0]])   # the first group's (first) parity is lost
                n_late += old_par is not None
    return streams, lists, n_late


def _restated(streams, lists, G, seq_base):
    """The documented order, restated: every part is the G items' arrays one after the other."""
    parts, late = [], []
    for s, (info, _) in enumerate(streams):
        got = [packets.gather(lists[s][i], info, seq_base=seq_base, late=late) for i in range(G)]
        parts += [np.concatenate([g[0].reshape(-1) for g in got]), np.concatenate([g[1].reshape(-1) for g in got])]
    for s, (info, fec) in enumerate(streams):
        if fec is not None:
            got = [packets.gather_fec(lists[2 + s][i], info, fec, seq_base=seq_base // fec.group, late=late) for i in range(G)]
            parts += [np.concatenate([g[0].reshape(-1) for g in got]), np.concatenate([g[1].reshape(-1) for g in got])]
    return parts, len(late)


@pytest.mark.parametrize("seq_base", [0, 16])
@pytest.mark.parametrize("n", [16, 3, 40])
@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("name", list(OPTIONS))
def test_the_front_end_builds_the_documented_layout(name, G, n, seq_base, cpu_net):
    opt = OPTIONS[name]
    streams, lists, n_late = _items(opt, G, n, seq_base, seed=1000 * G + 10 * n + seq_base + len(name))
    parts, late_want = _restated(streams, lists, G, seq_base)
    want = np.concatenate(parts)
    assert late_want == n_late and (n_late > 0) == (seq_base > 0)
    front = stream._RxFront(K, NB, PTOK, **opt)
    lay = front.layout(G, n)
    at = [int(v) for v in np.cumsum([0] + [p.size for p in parts])]
    assert lay.P == streams[0][0].P == -(-n // PTOK) and lay.size == at[-1] and (lay.bodies, lay.counts) == (at[0], at[1])
    k = 2
    if "audio" in opt:
        assert (lay.abodies, lay.acounts) == (at[2], at[3])
        k = 4
    else:
        assert lay.abodies is None and lay.acounts is None
    for f, got in ((opt.get("fec"), lay.fec), (opt.get("audio_fec"), lay.audio_fec)):
        assert got == (None if f is None else (at[k], at[k + 1]))
        k += 0 if f is None else 2
    assert k == len(parts)
    host, late = np.full(lay.size, 0xEE, np.uint8), []
    for i in reversed(range(G)):                                             # any order: an item's place depends on i alone
        item = front.gather_item(*(pk[i] for pk in lists), n, seq_base=seq_base, late=late)
        assert len(item) == len(parts) and all(p.size * G == q.size for p, q in zip(item, parts))
        front.fill(host, lay, i, item)
    assert np.array_equal(host, want) and len(late) == n_late
    if seq_base:                                                             # without a ``late`` list a stale packet is refused, as in packets.gather
        with pytest.raises(ValueError, match="seq"):
            front.gather_item(*(pk[0] for pk in lists), n, seq_base=seq_base)
    if n <= 16:                                                              # the lockstep receiver's chunk: the same bytes
        rx = cpu_net.stream_receiver(K, NB, batch=G, **opt)
        rx.tokens = PTOK * seq_base
        codes_or_apk = lists[1] if "audio" in opt else None
        host = rx._gather(lists[0], n, codes_or_apk, lists[2] if "fec" in opt else None, lists[3] if "audio_fec" in opt else None)
        assert host.dtype == np.uint8 and np.array_equal(host, want) and rx.late == n_late and rx._layout(G, n) == lay


def test_the_plain_pool_uploads_the_bytes_it_always_did(cpu_net):
    pool = cpu_net.stream_receiver_pool(K, NB, slots=5)
    sids = [pool.open() for _ in range(4)]
    pool.close(sids[1])                                                      # slots 0, 2, 3 stay: the slot lists are not 0, 1, 2
    a, b, c = sids[0], sids[2], sids[3]
    pool._sess[a][1] = pool._sess[c][1] = 32                                 # a and c take a steady chunk, b ends on 5 tokens
    rng = np.random.default_rng(11)
    codes = torch.zeros(32, 16, dtype=torch.int64)
    arrived = {}
    for sid, n, base in ((a, 16, 16), (b, 5, 0), (c, 16, 16)):
        pk, _ = _sent(rng, StreamInfo(K, NB, n, PTOK), None, base)
        arrived[sid] = _arrived(pk, sid, None)
    work = pool._inputs({a: (arrived[a], codes), c: (arrived[c], codes)}, {b: (arrived[b], codes[:, :5])})
    groups, slot_lists, where, host = pool._upload(work)
    assert [g.sids for g in groups] == [(b,), (a, c)] and slot_lists == [[2], [0, 3]]
    # restated: the slot lists (int32), then per group the bodies [G, P, full] and the counts [G, P]
    full = packets.body_bytes(PTOK, NB, K)
    want = [np.asarray([2, 0, 3], np.int32).view(np.uint8)]
    size = 12
    for members, n, base in (((b,), 5, 0), ((a, c), 16, 16)):
        G, P = len(members), (n + PTOK - 1) // PTOK
        got = [packets.gather(arrived[s], StreamInfo(K, NB, n, PTOK), seq_base=base) for s in members]
        hb, hc = np.stack([g[0] for g in got]), np.stack([g[1] for g in got])
        assert hb.shape == (G, P, full) and hc.shape == (G, P)
        want += [hb.reshape(-1), hc.reshape(-1)]
        size += G * P * (full + 1)
    want = np.concatenate(want)
    assert host.dtype == np.uint8 and host.size == size == want.size and np.array_equal(host, want)
    assert [o for o, _ in where] == [12, 12 + 3 * (full + 1)] and where[1][1] == stream.receiver_layout(2, 16, full, None, None, None, PTOK)
    # a finisher without a last chunk takes no segment
    work = pool._inputs({a: (arrived[a], codes)}, {b: None})
    groups, slot_lists, where, host = pool._upload(work)
    assert [g.key[1] for g in groups] == [0, 16] and where[0] == (8, None) and host.size == 8 + 8 * (full + 1)
