"""-m gpu: the receiver front end (``stream._RxFront``) against the numpy side.  The whole-item, streaming and pool receivers all
unpack through it, so an equality between them no longer guards it: here the expected values come from packets.gather,
packets.fec_recover and packets.unpack_bodies alone, for each of the four option sets -- tactile only, audio packets, a Fec with
parity 1, a Fec with parity 2 together with an audio Fec.  B = 2 items of T = 19 tokens (one chunk and a 3-token tail: the last
packet is short); per item and stream one packet is lost and one thinned; item 1 also loses the parity of the group its lost
packet is in, so that packet stays lost.  Every comparison is an equality.  The first test needs no device: it checks that the
numpy side of the case is what this paragraph says."""
import numpy as np
import pytest
import torch

from multimodal_vqvae_compression_audio_tactile_amd import bitstream, packets, stream
from multimodal_vqvae_compression_audio_tactile_amd.packets import Fec, StreamInfo

K, NB, KA, NA, PTOK, B, T = 512, 8, 1024, 32, 2, 2, 19
OPTIONS = {"tactile": {}, "audio": dict(audio=(KA, NA)), "fec1": dict(fec=Fec(4, 3)),
           "fec2+afec": dict(audio=(KA, NA), fec=Fec(4, 3, 2), audio_fec=Fec(8, 4, 2))}


def _stream_case(rng, info, fec):
    """One stream of B items over the channel -> (sent indices [nb, B, T], arrived packets and parity packets per item, and what
    the numpy rule makes of them: idx [nb, B, T], valid [B, T])."""
    sent = rng.integers(0, info.K, size=(info.nb, B, info.T))
    rx, rx_par, idx, valid = [], [], [], []
    for b in range(B):
        bodies = packets.pack_bodies(sent[:, b], info)
        pk = packets.frame(bodies, info)
        lost, thinned = 1 + 4 * b, 9 - b                                     # item 0: packets 1 and 9 (the short one); item 1: 5 and 8
        pk[thinned] = packets.thin(pk[thinned], 2, info)
        rx.append([p for s, p in enumerate(pk) if s != lost][::-1])
        got_b, got_r = packets.gather(rx[b], info)
        if fec is not None:
            par = packets.frame_fec(packets.fec_rows(bodies, None, info, fec), info, fec)
            if b == 1:                                                       # the parity of the lost packet's group does not arrive
                par = [p for p in par if packets._HEADER.unpack_from(p)[2] != lost // fec.group]
            rx_par.append(par)
            got_b, got_r, recovered = packets.fec_recover(got_b, got_r, *packets.gather_fec(par, info, fec), info, fec)
            assert recovered.tolist() == [int(s == thinned or (s == lost and b == 0)) for s in range(info.P)]
        i_b, v_b = packets.unpack_bodies(got_b, got_r, info)
        idx.append(i_b), valid.append(v_b)
    return sent, rx, rx_par if fec is not None else None, np.stack(idx, axis=1), np.stack(valid).astype(np.uint8)


def _case(name):
    opt, rng = OPTIONS[name], np.random.default_rng(len(name))
    tact = _stream_case(rng, StreamInfo(K, NB, T, PTOK), opt.get("fec"))
    audio = _stream_case(rng, StreamInfo(*opt["audio"], T, PTOK), opt.get("audio_fec")) if "audio" in opt else None
    return opt, tact, audio


@pytest.mark.parametrize("name", list(OPTIONS))
def test_the_numpy_side_sees_a_loss_a_thinning_and_a_recovery(name):
    """No device: what the case below feeds is what its docstring says."""
    opt, tact, audio = _case(name)
    for (sent, _, par, idx, valid), nb, fec in ((tact, NB, opt.get("fec")),) + (((audio, NA, opt.get("audio_fec")),) if audio else ()):
        v0, v1 = valid[0].tolist(), valid[1].tolist()
        m = 0 if fec is None else fec.books                                  # a recovered packet comes back at its protected books
        assert v0 == [nb] * 2 + [m] * 2 + [nb] * 14 + [max(2, m)] and v1 == [nb] * 10 + [0] * 2 + [nb] * 4 + [max(2, m)] * 2 + [nb]
        assert (par is None) == (fec is None)
        for b in range(B):
            for t in range(T):
                assert np.array_equal(idx[:valid[b, t], b, t], sent[:valid[b, t], b, t])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(OPTIONS))
def test_unpack_and_the_whole_item_calls_equal_the_numpy_side(name, dev):
    from test_gpu_av import _net
    opt, tact, audio = _case(name)
    none = [None] * B
    lists = [tact[1], none if audio is None else audio[1], tact[2] or none, none if audio is None else audio[2] or none]
    front = stream._RxFront(K, NB, PTOK, **opt)
    lay = front.layout(B, T)
    host = np.empty(lay.size, np.uint8)
    for b in range(B):
        front.fill(host, lay, b, front.gather_item(*(pk[b] for pk in lists), T))
    idx, nbv, codes, nav = front.unpack(torch.from_numpy(host).to(dev), lay, B, T)
    assert idx.dtype == torch.int64 and nbv.dtype == torch.uint8
    assert np.array_equal(idx.cpu().numpy(), tact[3]) and np.array_equal(nbv.cpu().numpy(), tact[4])
    if audio is None:
        assert codes is None and nav is None
    else:
        assert codes.is_contiguous() and np.array_equal(codes.cpu().numpy(), audio[3].transpose(1, 0, 2))
        assert np.array_equal(nav.cpu().numpy(), audio[4])
    # the whole-item calls: what is still lost after recovery
    net = _net(dev)
    infos, fec_kw = [StreamInfo(K, NB, T, PTOK)] * B, {}
    if "fec" in opt:
        fec_kw = dict(fec=opt["fec"], fec_packets=tact[2])
    if audio is None:
        payloads = [bitstream.pack_indices(np.zeros((NA, T), np.int64), KA)] * B
        y, lost = net.decompress_packets(infos, tact[1], payloads, **fec_kw)
    else:
        if "audio_fec" in opt:
            fec_kw.update(audio_fec=opt["audio_fec"], audio_fec_packets=audio[2])
        y, lost, alost = net.decompress_packets_av(infos, tact[1], [StreamInfo(KA, NA, T, PTOK)] * B, audio[1], **fec_kw)
        assert alost.dtype == torch.bool and np.array_equal(alost.cpu().numpy(), audio[4] == 0)
    assert y.shape == (B, 1, 320 * T - 8) and lost.dtype == torch.bool and np.array_equal(lost.cpu().numpy(), tact[4] == 0)
    assert bool(lost[1].any()) and bool(lost[0].any()) == ("fec" not in opt)
