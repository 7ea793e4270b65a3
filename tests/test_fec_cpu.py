"""CPU: forward error correction as packets.py defines it (fec_rows / frame_fec / gather_fec / fec_recover), against the existing
frame / thin / gather / unpack_bodies, on the six shapes of tests/fec_channel.py over seeded channels that drop, thin, reorder and
duplicate data packets and drop parity.

  * a recovered row is the body of thin(sent_packet, c_q), zero-padded; an unrecovered group is untouched;
  * after unpack_bodies every book counted in nb_valid is the index that was sent;
  * the frame_fec -> gather_fec round trip and its length formula; every refusal;
  * THE CONDITION the GPU tests rely on: the seeded channels produce each of the four outcomes;
  * the new symbols are exported and refuse bad shapes before any launch; the Python surface has the new arguments, the pools
    do not."""
import inspect
import struct

import numpy as np
import pytest

import fec_channel as fc
from multimodal_vqvae_compression_audio_tactile_amd import packets
from multimodal_vqvae_compression_audio_tactile_amd.packets import Fec, StreamInfo



def _zero_padded(body, width):
    out = np.zeros(width, np.uint8)
    out[:len(body)] = np.frombuffer(body, np.uint8)
    return out


@pytest.mark.parametrize("shape", fc.SHAPES)
def test_the_rule_on_seeded_channels(shape):
    seen = set()
    for seed in range(max(12, 200 // StreamInfo(*shape[:4]).P)):            # a one-packet item needs more channels to see everything
        it = fc.item(shape, seed)
        info, fec = it["info"], it["fec"]
        g, m, G, W = fec.resolve(info)
        full = packets.body_bytes(info.packet_tok, info.nb, info.K)
        recv, recv_par = fc.channel(it["sent"], it["par"], info, 77 * seed + 5)
        o = fc.rule(recv, recv_par, info, fec)
        seen |= fc.outcomes(it["nb_sent"], o["r0"], o["got"], info, fec)
        for j in range(G):
            grp = list(range(j * g, min(info.P, (j + 1) * g)))
            if not o["rec"][grp].any():                                   # an unrecovered group is untouched
                assert np.array_equal(o["b1"][grp], o["b0"][grp]) and np.array_equal(o["r1"][grp], o["r0"][grp])
                continue
            assert o["got"][j] and o["rec"][grp].sum() == 1
            q = grp[int(np.argmax(o["rec"][grp]))]
            c_q = min(m, int(it["nb_sent"][q]))
            assert o["r0"][q] < c_q == o["r1"][q]
            thinned = packets.thin(it["sent"][q], c_q, info)
            assert np.array_equal(o["b1"][q], _zero_padded(thinned[packets.HEADER_BYTES:], full))
            rest = [p for p in grp if p != q]
            assert np.array_equal(o["b1"][rest], o["b0"][rest]) and np.array_equal(o["r1"][rest], o["r0"][rest])
        idx, nb_valid = packets.unpack_bodies(o["b1"], o["r1"], info)
        for t in range(info.T):                                           # every book that counts is the index sent
            assert np.array_equal(idx[:nb_valid[t], t], it["idx"][:nb_valid[t], t]), (seed, t)
        assert (nb_valid > 0).sum() >= (packets.unpack_bodies(o["b0"], o["r0"], info)[1] > 0).sum()
    want = set(fc.OUTCOMES) - ({"two-deficient"} if shape[4] == 1 else set())      # a group of one cannot have two deficient
    assert seen == want, (shape, seen)


def test_every_outcome_occurs_in_the_family():
    """The condition, not a measurement: over the six shapes the channels of these tests produce all four outcomes."""
    seen = set()
    for shape in fc.SHAPES:
        for seed in range(3):                                             # the seeds tests/test_gpu_fec.py uses (B <= 3 items)
            it = fc.item(shape, seed)
            recv, recv_par = fc.channel(it["sent"], it["par"], it["info"], 77 * seed + 5)
            o = fc.rule(recv, recv_par, it["info"], it["fec"])
            seen |= fc.outcomes(it["nb_sent"], o["r0"], o["got"], it["info"], it["fec"])
    assert seen == set(fc.OUTCOMES)


@pytest.mark.parametrize("shape", fc.SHAPES)
def test_frame_gather_round_trip_and_length(shape):
    it = fc.item(shape, 3)
    info, fec = it["info"], it["fec"]
    g, m, G, W = fec.resolve(info)
    assert it["rows"].shape == (G, g + W) and W == packets.body_bytes(info.packet_tok, m, info.K) and len(it["par"]) == G
    bits = 0
    for j, pkt in enumerate(it["par"]):
        grp = range(j * g, min(info.P, (j + 1) * g))
        c = [min(m, int(it["nb_sent"][p])) for p in grp]
        n = max(packets.body_bytes(info.ntok(p), cp, info.K) for p, cp in zip(grp, c))
        assert len(pkt) == packets.HEADER_BYTES + len(grp) + n
        assert struct.unpack_from("<2sBIBB", pkt) == (b"MF", packets.VERSION, j, len(grp), max(c))
        assert list(pkt[9:9 + len(grp)]) == c and not it["rows"][j, g + n:].any() and not it["rows"][j, len(grp):g].any()
        bits += 8 * len(pkt)
    assert packets.fec_bits(info, fec, it["nb_sent"]) == bits
    assert packets.fec_bits(info, fec, it["nb_sent"], headers=False) == bits - 8 * sum(9 + len(range(j * g, min(info.P, (j + 1) * g))) for j in range(G))
    assert packets.fec_kbps(info, fec, it["nb_sent"]) == bits * 75.0 / (1000.0 * info.T)
    rows, got = packets.gather_fec(it["par"][::-1] + it["par"][:1], info, fec)
    assert np.array_equal(rows, it["rows"]) and got.dtype == np.uint8 and got.all()
    rows, got = packets.gather_fec(it["par"][1:], info, fec)
    assert not got[0] and not rows[0].any() and np.array_equal(rows[1:], it["rows"][1:])
    # the streaming numbers: seq_base and late, as gather has them
    par7 = packets.frame_fec(it["rows"], info, fec, seq_base=7)
    late = []
    rows, got = packets.gather_fec(par7 + it["par"][:1], info, fec, seq_base=7, late=late)
    assert np.array_equal(rows, it["rows"]) and late == it["par"][:1]
    with pytest.raises(ValueError, match="seq_base"):
        packets.gather_fec(it["par"][:1], info, fec, seq_base=7)
    # nb_sent None / a scalar: every packet
    assert np.array_equal(packets.fec_rows(it["bodies"], None, info, fec), packets.fec_rows(it["bodies"], [info.nb] * info.P, info, fec))
    assert np.array_equal(packets.fec_rows(it["bodies"], 1, info, fec), packets.fec_rows(it["bodies"], [1] * info.P, info, fec))
    # a recovered packet IS a thinned packet: all parity, one packet lost per group
    keep = [p for s, p in enumerate(it["sent"]) if s % g != 0]
    o = fc.rule(keep, it["par"], info, fec)
    for q in range(0, info.P, g):
        assert o["rec"][q] and o["r1"][q] == min(m, it["nb_sent"][q])
    # parity for a group with nothing missing changes nothing
    o = fc.rule(it["sent"], it["par"], info, fec)
    assert not o["rec"].any() and np.array_equal(o["b1"], o["b0"]) and np.array_equal(o["r1"], it["nb_sent"])
    # a data packet is refused by gather_fec and a parity packet by gather, by their magic
    with pytest.raises(ValueError, match="magic"):
        packets.gather(it["par"][:1], info)
    with pytest.raises(ValueError, match="magic"):
        packets.gather_fec(it["sent"][:1], info, fec)


def test_refusals():
    info = StreamInfo(512, 8, 37, 2)
    for bad in (Fec(0, 3), Fec(17, 3), Fec(4, 0), Fec(4, 9)):
        with pytest.raises(ValueError, match="Fec"):
            bad.resolve(info)
    with pytest.raises(ValueError, match="K = 1"):
        Fec(4, 3).resolve(StreamInfo(1, 8, 37, 2))
    with pytest.raises(ValueError, match="not an integer"):
        Fec(4.0, 3)
    with pytest.raises(ValueError, match="not an integer"):
        Fec(4, True)
    assert Fec(4, 3).resolve(info) == (4, 3, 5, 7) and Fec(16, 8).resolve(info) == (16, 8, 2, 18)
    assert Fec(4, 3).resolve(info, chunk_tok=16) == (4, 3, 5, 7) and Fec(8, 3).resolve(info, chunk_tok=16)[0] == 8
    for bad in (Fec(3, 3), Fec(16, 3)):                                    # 8 packets per chunk
        with pytest.raises(ValueError, match="chunk"):
            bad.resolve(info, chunk_tok=16)
    with pytest.raises(dataclass_frozen_error()):
        Fec(4, 3).group = 5
    it = fc.item(fc.SHAPES[0], 1)
    info, fec, par = it["info"], it["fec"], it["par"]
    p = par[1]
    for bad, what in ((b"MP" + p[2:], "magic"), (p[:2] + b"\x02" + p[3:], "version"), (p[:3] + struct.pack("<I", 5) + p[7:], "seq"),
                      (p[:7] + b"\x03" + p[8:], "covers"), (p[:8] + b"\x07" + p[9:], "counts"), (p[:9] + b"\x00" + p[10:], "counts"),
                      (p[:9] + b"\x04" + p[10:], "counts"), (p + b"\x00", "bytes"), (p[:-1], "bytes"), (p[:5], "shorter"),
                      (p[:10], "shorter|bytes")):
        with pytest.raises(ValueError, match=what):
            packets.gather_fec([bad], info, fec)
    with pytest.raises(ValueError, match="parity rows"):
        packets.frame_fec(it["rows"][:-1], info, fec)
    bad_rows = it["rows"].copy()
    bad_rows[0, 0] = 0
    with pytest.raises(ValueError, match="count"):
        packets.frame_fec(bad_rows, info, fec)
    with pytest.raises(ValueError, match="seq_base"):
        packets.frame_fec(it["rows"], info, fec, seq_base=2 ** 32 - 2)
    with pytest.raises(ValueError, match="counts"):
        packets.fec_rows(it["bodies"], it["nb_sent"][:-1], info, fec)
    with pytest.raises(ValueError, match="fec_recover"):
        packets.fec_recover(it["bodies"], it["nb_sent"], it["rows"][:-1], np.ones(4), info, fec)


def dataclass_frozen_error():
    import dataclasses
    return dataclasses.FrozenInstanceError


def test_a_corrupt_count_is_clamped_and_more_deficient_packets_leave_the_group_alone():
    it = fc.item(fc.SHAPES[0], 2)
    info, fec = it["info"], it["fec"]
    bodies, r0 = packets.gather(it["sent"][1:], info)                      # packet 0 lost
    rows, got = it["rows"].copy(), np.ones(len(it["par"]), np.uint8)
    want = packets.fec_recover(bodies, r0, rows, got, info, fec)
    assert want[2][0] == 1
    rows[0, 0] = 255                                                       # corrupt: counts as min(255, m, nb) = m
    b1, r1, rec = packets.fec_recover(bodies, r0, rows, got, info, fec)
    assert rec[0] == 1 and r1[0] == 3 and b1.shape == bodies.shape
    r2 = r0.copy()
    r2[1] = 0                                                              # two deficient: untouched
    b1, r1, rec = packets.fec_recover(bodies, r2, it["rows"], got, info, fec)
    assert not rec[:4].any() and np.array_equal(b1, bodies) and np.array_equal(r1, r2)
    b1, r1, rec = packets.fec_recover(bodies, r0, it["rows"], np.zeros_like(got), info, fec)
    assert not rec.any() and np.array_equal(b1, bodies) and np.array_equal(r1, r0)


def test_entry_points_are_exported_and_refuse_before_any_launch():
    from multimodal_vqvae_compression_audio_tactile_amd import ProposedEval, StreamReceiver, StreamSender, _lib
    lib = _lib.lib()
    for n in ("mvq_fec_parity_u8", "mvq_fec_recover_u8"):
        assert n in _lib.EXPORTS and hasattr(lib, n), n
    assert lib.mvq_abi_version() == 3

    def parity(batch=1, nb=8, t=37, k=512, ptok=2, g=4, m=3):
        return lib.mvq_fec_parity_u8(None, None, None, batch, nb, t, k, ptok, g, m, None)

    def recover(batch=1, nb=8, t=37, k=512, ptok=2, g=4, m=3):
        return lib.mvq_fec_recover_u8(None, None, None, None, None, batch, nb, t, k, ptok, g, m, None)

    for call, who in ((parity, b"fec_parity:"), (recover, b"fec_recover:")):
        assert call() == -1 and lib.mvq_last_error().startswith(who) and b"null" in lib.mvq_last_error()   # a good shape gets to the tensors
        assert call(batch=0) == 0 and call(t=0) == 0                       # empty: a no-op
        for kw in (dict(g=0), dict(g=17), dict(m=0), dict(m=9), dict(nb=0), dict(batch=-1), dict(t=-1), dict(k=0), dict(ptok=0),
                   dict(ptok=256), dict(nb=256), dict(k=2 ** 25), dict(g=0, batch=0), dict(m=9, t=0)):
            assert call(**kw) == -1 and b"bad shape" in lib.mvq_last_error(), kw
    for fn in (ProposedEval.compress_packets, ProposedEval.decompress_packets, ProposedEval.compress_packets_av,
               ProposedEval.decompress_packets_av, StreamSender.__init__, StreamReceiver.__init__, ProposedEval.stream_sender,
               ProposedEval.stream_receiver):
        assert inspect.signature(fn).parameters["fec"].default is None, fn
    for fn in (ProposedEval.compress_packets_av, ProposedEval.decompress_packets_av, StreamSender.__init__, StreamReceiver.__init__):
        assert inspect.signature(fn).parameters["audio_fec"].default is None, fn
    for fn in (StreamReceiver.push, StreamReceiver.finish):
        assert inspect.signature(fn).parameters["fec_packets"].default is None
        assert inspect.signature(fn).parameters["audio_fec_packets"].default is None
    for fn in (ProposedEval.stream_sender_pool, ProposedEval.stream_receiver_pool):      # the pools take no fec
        assert "fec" not in inspect.signature(fn).parameters


def test_ops_refuse_what_is_not_on_the_device():
    import torch
    from multimodal_vqvae_compression_audio_tactile_amd import MvqError, ops
    info, fec = StreamInfo(512, 8, 37, 2), Fec(4, 3)
    bodies, counts = torch.zeros(1, 19, 18, dtype=torch.uint8), torch.zeros(1, 19, dtype=torch.uint8)
    with pytest.raises(MvqError, match="bodies"):
        ops.fec_parity(bodies, None, info, fec)
    with pytest.raises(MvqError, match="bodies"):
        ops.fec_recover(bodies, counts, torch.zeros(1, 5, 11, dtype=torch.uint8), torch.zeros(1, 5, dtype=torch.uint8), info, fec)
    for bad in (Fec(0, 3), Fec(17, 3), Fec(4, 9)):
        with pytest.raises(MvqError, match="group"):
            ops.fec_parity(bodies, None, info, bad)
    with pytest.raises(MvqError, match="StreamInfo"):
        ops.fec_parity(bodies, None, info, (4, 3))
