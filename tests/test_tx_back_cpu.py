"""No GPU: the sender back end (``stream._TxBack``), the one owner of the read-back's format.  The whole-item
calls, the lockstep sender and both pools all pack and frame through it, so an equality between them no longer guards the format:
here every expected value comes from the numpy side alone (packets.pack_bodies / fec_rows / frame / frame_fec).

  1. layout and framing: ``layout(n)`` against a plain running sum of the sizes of pack_bodies, the counts and fec_rows, and
     ``frame_item`` on a row built by plain concatenation against packets.frame(seq_base) / frame_fec(seq_base // group);
  2. the return-shape glue: ``_nothing`` and ``_infos`` against a real result, for StreamSender(batch=2) and both pools.

Every comparison is an equality.  ``numpy_item`` also serves tests/test_gpu_tx_back.py."""
import numpy as np
import pytest
import torch

from multimodal_vqvae_compression_audio_tactile_amd import packets, stream
from multimodal_vqvae_compression_audio_tactile_amd.packets import Fec, Rate, StreamInfo

K, NB, KA, NA, PTOK = 512, 8, 1024, 32, 2
# the four option sets of tests/test_gpu_rx_front.py, and tactile-only and fec1 with the counts behind the bodies
OPTIONS = {"tactile": {}, "tactile+counts": dict(counts=True), "audio": dict(audio=(KA, NA)), "fec1": dict(fec=Fec(4, 3)),
           "fec1+counts": dict(counts=True, fec=Fec(4, 3)),
           "fec2+afec": dict(audio=(KA, NA), fec=Fec(4, 3, 2), audio_fec=Fec(8, 4, 2))}


@pytest.fixture(scope="module")
def cpu_net():
    from multimodal_vqvae_compression_audio_tactile_amd import build_proposed
    return build_proposed(None, rvq_books=NB, rvq_embed=K, device="cpu")


def numpy_item(rng, opt, n):
    """One item of ``n`` tokens under ``opt`` (_TxBack's options), the numpy side alone -> (per stream (info, fec, idx [nb, n],
    bodies, counts [P] or None, parity rows or None), the row's parts in the documented order: per stream the bodies and, with
    counts, the counts; then per stream with a Fec its parity rows).  The counts are drawn from 1..nb."""
    counted = bool(opt.get("counts")) or "audio" in opt
    streams = [(StreamInfo(K, NB, n, PTOK), opt.get("fec"))] + ([(StreamInfo(*opt["audio"], n, PTOK), opt.get("audio_fec"))] if "audio" in opt else [])
    out = []
    for info, fec in streams:
        idx = rng.integers(0, info.K, size=(info.nb, n))
        bodies = packets.pack_bodies(idx, info)
        sent = rng.integers(1, info.nb + 1, size=info.P).astype(np.uint8) if counted else None
        out.append((info, fec, idx, bodies, sent, None if fec is None else packets.fec_rows(bodies, sent, info, fec)))
    parts = [p for _, _, _, bodies, sent, _ in out for p in ((bodies, sent) if counted else (bodies,))]
    parts += [rows for *_, rows in out if rows is not None]
    return out, [np.asarray(p, np.uint8).reshape(-1) for p in parts]


def framed_by_numpy(item, seq_base):
    """What ``frame_item`` documents, from packets.frame / frame_fec alone."""
    want = tuple(packets.frame(bodies, info, nb_sent=sent, seq_base=seq_base) for info, _, _, bodies, sent, _ in item)
    if all(fec is None for _, fec, *_ in item):
        return want
    return want + tuple([] if fec is None else packets.frame_fec(rows, info, fec, seq_base=seq_base // fec.group)
                        for info, fec, _, _, _, rows in item)


# ------------------------------------------------------------------------------------------------- 1. layout and framing
@pytest.mark.parametrize("n", [19, 16])                 # 19: one chunk and a 3-token tail -- a short last packet, and the last
@pytest.mark.parametrize("name", list(OPTIONS))         # parity group of 4 and the last of 8 hold 2 packets each
def test_layout_and_framing_equal_the_numpy_side(name, n):
    opt = OPTIONS[name]
    item, parts = numpy_item(np.random.default_rng(4000 + 100 * n + len(name)), opt, n)   # a seed whose counts pass the check below
    for info, fec, _, _, sent, _ in item:
        assert info.P == -(-n // PTOK) and info.ntok(info.P - 1) == (1 if n == 19 else 2)
        if fec is not None:
            assert info.P - (info.P - 1) // fec.group * fec.group == (2 if n == 19 else fec.group)       # the last group's packets
            if sent is not None:                                             # min(books, count) goes both ways
                assert (sent < fec.books).any() and (sent > fec.books).any()
    back = stream._TxBack(K, NB, PTOK, **opt)
    at = [0]
    for p in parts:                                                          # a plain running sum
        at.append(at[-1] + p.size)
    assert back.layout(n) == tuple(zip(at[:-1], at[1:])) and len(parts) == {"tactile": 1, "tactile+counts": 2, "audio": 4, "fec1": 2,
                                                                            "fec1+counts": 3, "fec2+afec": 6}[name]
    row = np.concatenate(parts)
    for seq_base in (0, 16):
        assert back.frame_item(row, n, seq_base) == framed_by_numpy(item, seq_base), seq_base
    assert back.frame_item(row.reshape(1, -1), n) == framed_by_numpy(item, 0)
    with pytest.raises(ValueError, match="frame_item"):                      # a row of another option set or length is refused, not cut
        back.frame_item(row[:-1], n)
    with pytest.raises(ValueError, match="frame_item"):
        back.frame_item(np.concatenate([row, row[:1]]), n)


# ---------------------------------------------------------------------------------------------- 2. the return-shape glue
SENDER_CASES = [dict(rate=Rate(min_books=2, tol2=0.84), audio="packets", fec=Fec(4, 3), audio_fec=Fec(8, 4, 2)),
                dict(audio="packets", audio_fec=Fec(8, 4, 2)), dict(audio="packets"),
                dict(rate=Rate(min_books=2, tol2=0.84), audio="codes", fec=Fec(4, 3)), dict(audio="codes", fec=Fec(8, 3, 2)),
                dict(rate=Rate(budget=27), audio="codes"), dict(audio="codes")]


def _shape(result):
    """The length and list positions of a result: per element, list or not."""
    return [isinstance(v, list) for v in result]


@pytest.mark.parametrize("kw", SENDER_CASES, ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_nothing_and_infos_have_the_places_of_a_real_result(kw, cpu_net):
    n, T = 16, 53
    packets_on = kw["audio"] == "packets"
    opt = dict(counts=kw.get("rate") is not None, fec=kw.get("fec"), audio_fec=kw.get("audio_fec"), **(dict(audio=(KA, NA)) if packets_on else {}))
    rng = np.random.default_rng(len(kw))
    items = [numpy_item(rng, opt, n) for _ in range(2)]
    rows = [np.concatenate(parts) for _, parts in items]
    infos = (StreamInfo(K, NB, T, PTOK),) + ((StreamInfo(KA, NA, T, PTOK),) if packets_on else ())
    n_real = 2 + (0 if opt["fec"] is None and opt["audio_fec"] is None else 2 if packets_on else 1)
    without_codes = (lambda r: r) if packets_on else (lambda r: (r[0],) + tuple(r[2:]))
    # the lockstep sender: every value a list per item
    tx = cpu_net.stream_sender(batch=2, **kw)
    codes = torch.zeros(2, 32, n, dtype=torch.int64)
    real, nothing = tx._framed(torch.from_numpy(np.stack(rows)), codes, n), tx._nothing()
    assert without_codes(real) == tuple(list(c) for c in zip(*(framed_by_numpy(item, 0) for item, _ in items)))
    assert len(real) == n_real and _shape(nothing) == _shape(real)
    assert all(v == [[], []] for v in nothing if isinstance(v, list))
    if not packets_on:
        assert real[1] is codes and nothing[1].shape == (2, 32, 0) and nothing[1].dtype == torch.int64
    assert tx._infos(T) == infos and tx._finished(real, T) == tuple(real[:2]) + infos + tuple(real[2:])
    assert _shape(tx._finished(nothing, T)) == _shape(tx._finished(real, T))
    # the pools: one item's values, the session at chunk 1
    pools = [cpu_net.stream_sender_pool_av(slots=2, **kw)] + ([cpu_net.stream_sender_pool(slots=2)] if kw == dict(audio="codes") else [])
    one = codes[:1]
    for pool in pools:
        real, nothing = pool._frame(rows[0], n, 1, one), pool._nothing()
        assert without_codes(real) == framed_by_numpy(items[0][0], 8)
        assert len(real) == n_real and _shape(nothing) == _shape(real) and all(v == [] for v in nothing if isinstance(v, list))
        if not packets_on:
            assert real[1] is one and nothing[1].shape == (1, 32, 0) and nothing[1].dtype == torch.int64
        assert pool._infos(T) == infos and pool._finished(real, T) == tuple(real[:2]) + infos + tuple(real[2:])
