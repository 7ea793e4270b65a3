"""-m gpu: the sender back end (``stream._TxBack``) against the numpy side.  The whole-item calls, the
lockstep sender and the pools all pack through it, so an equality between them no longer guards it: here the expected bytes come
from packets.pack_bodies / fec_rows / frame / frame_fec alone, for the option sets of tests/test_tx_back_cpu.py, B = 2 items of
T = 19 tokens (one chunk and a 3-token tail: the last packet is short, the last parity groups hold 2 packets).

  1. the device half: seeded indices, codes and counts through ``pack`` -> per item the plain concatenation of the numpy parts; a
     row of a single part is the packed bodies themselves, a view;
  2. the whole-item calls: compress_packets / compress_packets_av return packets.frame / frame_fec of what
     encode_latents_with_indices (deterministic) gives under the same options;
  3. the carry rule: a pool session that finishes in the tick of another session's push, and the session that takes its slot.

Every comparison is an equality."""
import numpy as np
import pytest
import torch

from multimodal_vqvae_compression_audio_tactile_amd import bitstream, packets, stream, synth
from multimodal_vqvae_compression_audio_tactile_amd.packets import Fec, Rate, StreamInfo
from test_tx_back_cpu import K, KA, NA, NB, OPTIONS, PTOK, framed_by_numpy, numpy_item

pytestmark = pytest.mark.gpu

B, T = 2, 19


# ------------------------------------------------------------------------------------------------------ 1. the device half
@pytest.mark.parametrize("name", list(OPTIONS))
def test_pack_equals_the_concatenated_numpy_parts(name, dev):
    opt, rng = OPTIONS[name], np.random.default_rng(len(name))
    items = [numpy_item(rng, opt, T) for _ in range(B)]
    up = lambda xs, axis: torch.from_numpy(np.stack(xs, axis=axis)).to(dev)
    counts = lambda s: None if items[0][0][s][4] is None else up([item[s][4] for item, _ in items], 0)
    idx = up([item[0][2] for item, _ in items], 1)                            # [nb, B, T]
    back = stream._TxBack(K, NB, PTOK, **opt)
    if "audio" in opt:
        codes = up([item[1][2] for item, _ in items], 0)                      # [B, 32, T]
        rows = back.pack(idx, counts(0), codes, counts(1))
    else:
        rows = back.pack(idx, counts(0))
    want = np.stack([np.concatenate(parts) for _, parts in items])
    assert rows.dtype == torch.uint8 and rows.shape == want.shape == (B, back.layout(T)[-1][1])
    assert np.array_equal(rows.cpu().numpy(), want)
    for b, (item, _) in enumerate(items):                                    # and the host half on the device's bytes
        assert back.frame_item(rows[b].cpu().numpy(), T, 16) == framed_by_numpy(item, 16)
    if name == "tactile":                                                    # a single part: the packed bodies, no copy
        P, full = items[0][0][0][0].P, packets.body_bytes(PTOK, NB, K)
        assert rows._base is not None and rows._base.shape == (B, P, full) and rows.data_ptr() == rows._base.data_ptr()
    else:
        assert rows._base is None


# -------------------------------------------------------------------------------------------------- 2. the whole-item calls
RATE, ARATE = Rate(min_books=2, tol2=0.84), Rate(min_books=2, tol2=0.5)


@pytest.mark.parametrize("name", list(OPTIONS))
def test_the_whole_item_calls_equal_the_numpy_side(name, dev):
    from test_gpu_av import _net
    net, opt = _net(dev), OPTIONS[name]
    a, t = synth.audio_segments(B, seed=19, T=320 * T).to(dev), synth.tactile_segments(B, seed=19, T=320 * T).to(dev)
    info, ainfo = StreamInfo(K, NB, T, PTOK), StreamInfo(KA, NA, T, PTOK)
    fec, afec = opt.get("fec"), opt.get("audio_fec")
    if "audio" in opt:
        got = net.compress_packets_av(a, t, rate=RATE, audio_rate=ARATE, fec=fec, audio_fec=afec)
        _, codes, idx, sent, asent = net.encode_latents_with_indices(a, t, rate=RATE, packet_tok=PTOK, audio_rate=ARATE)
        assert len(got) == (4 if fec is None and afec is None else 6)
    else:
        rate = RATE if opt.get("counts") else None
        got = net.compress_packets(a, t, rate=rate, **({} if fec is None else dict(fec=fec)))
        _, codes, idx, *sent = net.encode_latents_with_indices(a, t, rate=rate, packet_tok=PTOK)
        sent, asent = (sent[0] if sent else None), None
        assert len(got) == (3 if fec is None else 4)
    idx, codes = idx.cpu().numpy(), codes.cpu().numpy()
    assert idx.shape == (NB, B, T) and codes.shape == (B, NA, T)
    sent, asent = (None if s is None else s.cpu().numpy() for s in (sent, asent))
    assert got[0] == [info] * B
    for b in range(B):
        bodies = packets.pack_bodies(idx[:, b], info)
        nb_sent = None if sent is None else sent[b]
        assert got[1][b] == packets.frame(bodies, info, nb_sent=nb_sent)
        if "audio" not in opt:
            assert got[2][b] == bitstream.pack_indices(codes[b], KA)
            if fec is not None:
                assert got[3][b] == packets.frame_fec(packets.fec_rows(bodies, nb_sent, info, fec), info, fec)
            continue
        abodies = packets.pack_bodies(codes[b], ainfo)
        assert got[2] == [ainfo] * B and got[3][b] == packets.frame(abodies, ainfo, nb_sent=asent[b])
        if len(got) == 6:
            assert got[4][b] == packets.frame_fec(packets.fec_rows(bodies, nb_sent, info, fec), info, fec)
            assert got[5][b] == packets.frame_fec(packets.fec_rows(abodies, asent[b], ainfo, afec), ainfo, afec)


# ---------------------------------------------------------------------------------------------------------- 3. the carry rule
def _same(got, want):
    """A pool session's values against StreamSender(batch=1)'s: the one item's."""
    assert len(got) == len(want) and got[0] == want[0][0] and torch.equal(got[1], want[1]) and tuple(got[2:]) == tuple(want[2:])


def test_a_finishing_session_writes_no_carry_and_its_slot_starts_clean(dev):
    from test_gpu_av import _net
    net = _net(dev)
    sig = lambda seed, tok: (synth.audio_segments(1, seed=seed, T=320 * tok).to(dev), synth.tactile_segments(1, seed=seed, T=320 * tok).to(dev))
    cut = lambda x, lo, hi: tuple(v[..., 320 * lo:320 * hi] for v in x)
    xa, xb, xc = sig(3, 43), sig(4, 64), sig(5, 40)
    pool = net.stream_sender_pool(slots=2)
    solo = {k: net.stream_sender(batch=1) for k in "abc"}
    sa, sb = pool.open(), pool.open()
    slot = pool._sess[sa][0]
    for lo in (0, 16):                                                       # two chunks of samples each: the second push emits chunk 0
        out = pool.step({sa: cut(xa, lo, lo + 16), sb: cut(xb, lo, lo + 16)})
        _same(out[sa], solo["a"].push(*cut(xa, lo, lo + 16)))
        _same(out[sb], solo["b"].push(*cut(xb, lo, lo + 16)))
    # a finishes (27 tokens: chunks 1 and 2) in the tick in which b's push emits its chunk 1
    before = pool.carry[slot].clone()
    out = pool.step({sb: cut(xb, 32, 48)}, {sa: cut(xa, 32, 43)})
    assert [g.key[0] for g in pool.last_groups] == ["emit", "finish"]
    _same(out[sa], solo["a"].finish(*cut(xa, 32, 43)))
    _same(out[sb], solo["b"].push(*cut(xb, 32, 48)))
    assert out[sa][2] == StreamInfo(K, NB, 43, PTOK) and len(out[sa][0]) == 14 and pool.free == 1
    # the finishing tick wrote nothing into a's slot: it holds a's carried token of chunk 0, bit for bit, not chunk 2's; the
    # session that takes the slot starts from zero all the same
    assert bool(before.any()) and torch.equal(pool.carry[slot], before)
    sc = pool.open()
    assert pool._sess[sc][0] == slot and not bool(pool.carry[slot].any())
    for lo in (0, 16):
        out = pool.step({sc: cut(xc, lo, lo + 16), sb: cut(xb, 48 + lo // 2, 56 + lo // 2)})
        _same(out[sc], solo["c"].push(*cut(xc, lo, lo + 16)))
        _same(out[sb], solo["b"].push(*cut(xb, 48 + lo // 2, 56 + lo // 2)))
    out = pool.step({}, {sc: cut(xc, 32, 40), sb: None})
    _same(out[sc], solo["c"].finish(*cut(xc, 32, 40)))
    _same(out[sb], solo["b"].finish())
    assert pool.free == 2
