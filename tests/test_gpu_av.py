"""-m gpu: the audio transport (layered audio packets, closed-loop audio rate control) against the numpy restatement of
tests/av_oracle.py.  Every comparison is an equality.

  1. mvq_dac_rvq_from_codes_layers_f32 against the existing look-up on the prefix and against the restatement;
  2. mvq_dac_rvq_rate_f32: energies, counts and qa against the restatement, all three modes, packet_tok 1 / 2 / 16, a NaN token;
  3. through the model: encode_latents_with_indices(audio_rate=, rate=) against decode_latents(nb_valid=, na_valid=);
  4. the whole-item link: compress_packets_av / decompress_packets_av, lossless and over a seeded lossy channel;
  5. streaming: StreamSender(audio="packets") against compress_packets_av, into StreamReceiver(audio=) against decompress_packets_av;
  6. refusals before any launch."""
import numpy as np
import pytest
import torch

import av_oracle as av
import rate_oracle as rt
import sender_oracle as sn
from multimodal_vqvae_compression_audio_tactile_amd import packets, synth
from multimodal_vqvae_compression_audio_tactile_amd.packets import Rate, StreamInfo

pytestmark = pytest.mark.gpu

_NETS, _CASES = {}, {}
SHAPES = [(C, nq, K) for C in (128, 1024) for nq in (32, 9, 1) for K in (1024, 37)]
BT = [(1, 16), (3, 37), (2, 5)]
TOL2 = 1e-3                                     # tests/test_av_cpu.py: at least three distinct counts on these inputs


def _case(orc, C, nq, K, B, T):
    """Seeded quantiser and layered inputs with their stage outputs and energies, computed once per shape."""
    key = (C, nq, K, B, T)
    if key not in _CASES:
        q3 = av.quantiser(C + nq + K, nq=nq, K=K, C=C)
        z, codes, m_t = av.layered_inputs(orc, *q3, B, T, nq, seed=C + T + nq)
        zs = av.stages(orc, *q3, codes)
        _CASES[key] = (q3, z, codes, m_t, zs, av.energies(z, zs))
    return _CASES[key]


def _t(dev, *xs):
    return [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in xs]


# ------------------------------------------------------------------------------------------------- 1. layered from_codes
@pytest.mark.parametrize("B,T", BT)
@pytest.mark.parametrize("C,nq,K", SHAPES)
def test_layered_from_codes_kernel(C, nq, K, B, T, orc, dev):
    from multimodal_vqvae_compression_audio_tactile_amd import _lib, ops, torch_ops  # noqa: F401  (registers the operators)
    q3, _, codes, _, zs, _ = _case(orc, C, nq, K, B, T)
    assert codes.max() >= K and codes.min() < 0                                           # the clamp is exercised
    r = np.random.default_rng(C + nq + K + B + T)
    count = r.integers(0, nq + 6, size=(B, T)).astype(np.uint8)                           # 0 and values above nq
    count.reshape(-1)[:3] = (0, 255, nq)
    cb, ow, ob, cd, cnt = _t(dev, *q3, codes, count)
    zq, z_p = ops.dac_rvq_from_codes(cd, cb, ow, ob, nq_valid=cnt)
    assert zq.shape == (B, C, T) and z_p.shape == (B, nq * 8, T)
    raw = torch.full((B, C, T), float("nan"), device=dev)                                 # every element is written: garbage first
    rc = _lib.lib().mvq_dac_rvq_from_codes_layers_f32(cd.data_ptr(), nq * T, cb.data_ptr(), ow.data_ptr(), ob.data_ptr(), cnt.data_ptr(),
                                                      raw.data_ptr(), None, B, C, T, nq, K, 8, torch.cuda.current_stream().cuda_stream)
    assert rc == 0 and torch.equal(raw, zq)
    got = zq.cpu().numpy()
    assert np.array_equal(got, av.from_codes_layers(orc, *q3, codes, count, zs=zs))
    plain_q, plain_p = ops.dac_rvq_from_codes(cd, cb, ow, ob)
    assert torch.equal(z_p, plain_p)                                                      # the raw rows of all stages either way
    eff = np.minimum(count, nq)
    for m in sorted(set(eff.reshape(-1).tolist())):                                       # each column: the existing kernel on the prefix
        cols = eff == m
        want = np.zeros((B, C, T), np.float32) if m == 0 else ops.dac_rvq_from_codes(cd[:, :m].contiguous(), cb, ow, ob)[0].cpu().numpy()
        assert np.array_equal(got.transpose(0, 2, 1)[cols], want.transpose(0, 2, 1)[cols]), m
    zero = got.transpose(0, 2, 1)[eff == 0]
    assert zero.size and not np.signbit(zero).any()
    # nq_valid = None is the existing kernel; so is a count of nq everywhere
    assert torch.equal(ops.dac_rvq_from_codes(cd, cb, ow, ob, nq_valid=None)[0], plain_q)
    assert torch.equal(ops.dac_rvq_from_codes(cd, cb, ow, ob, nq_valid=torch.full_like(cnt, nq))[0], plain_q)
    assert torch.equal(torch.ops.mi355x_vqvae.dac_rvq_from_codes_layers(cd, cb, ow, ob, cnt)[0], zq)


def test_layered_from_codes_refusals(dev):
    from multimodal_vqvae_compression_audio_tactile_amd import MvqError, ops
    cb, ow, ob = _t(dev, *av.quantiser(1, nq=4, K=37, C=128))
    codes = torch.zeros(2, 4, 5, dtype=torch.int64, device=dev)
    for bad in (torch.zeros(2, 4, dtype=torch.uint8, device=dev), torch.zeros(2, 5, dtype=torch.int32, device=dev),
                torch.zeros(2, 5, dtype=torch.uint8), np.zeros((2, 5), np.uint8)):
        with pytest.raises(MvqError, match="nq_valid"):
            ops.dac_rvq_from_codes(codes, cb, ow, ob, nq_valid=bad)


# ------------------------------------------------------------------------------------------------- 2. the audio rate kernel
def _rates(nq, ptok):
    pc = 16 // ptok
    return {"full": Rate(), "tol2": Rate(tol2=TOL2), "tol2_min": Rate(min_books=min(nq, 3), tol2=TOL2),
            "budget": Rate(budget=pc * max(1, nq // 2) + (3 if nq > 1 else 0))}


def _want(orc, q3, codes, zs, E, rate, ptok, B, T):
    sent = np.stack([rt.decide(E[:, b], rate, ptok) for b in range(B)]).astype(np.uint8)
    valid = rt.expand(sent, T, ptok)
    return av.from_codes_layers(orc, *q3, codes, valid, zs=zs), valid, sent


@pytest.mark.parametrize("B,T", BT)                                                       # (3, 37) and (2, 5) end in a short tail group
@pytest.mark.parametrize("C,nq,K", SHAPES)
def test_audio_rate_kernel(C, nq, K, B, T, orc, dev):
    from multimodal_vqvae_compression_audio_tactile_amd import _lib, ops
    q3, z, codes, _, zs, E = _case(orc, C, nq, K, B, T)
    cb, ow, ob, zd, cd = _t(dev, *q3, z, codes)
    seen = set()
    for ptok in (1, 2, 16):
        for name, rate in _rates(nq, ptok).items():
            want_q, want_v, want_s = _want(orc, q3, codes, zs, E, rate, ptok, B, T)
            qa, nav, nas, en = ops.dac_rvq_rate(zd, cd, cb, ow, ob, rate, ptok, want_energy=True)
            assert qa.shape == (B, C, T) and nav.shape == (B, T) and nas.shape == (B, -(-T // ptok)) and en.shape == (nq + 1, B * T)
            assert np.array_equal(en.cpu().numpy().reshape(E.shape), E), (ptok, name)
            assert np.array_equal(nas.cpu().numpy(), want_s), (ptok, name)
            assert np.array_equal(nav.cpu().numpy(), want_v), (ptok, name)
            assert np.array_equal(qa.cpu().numpy(), want_q), (ptok, name)
            assert torch.equal(qa, ops.dac_rvq_from_codes(cd, cb, ow, ob, want_z_p=False, nq_valid=nav)[0])   # ... on the kernel's own counts
            if name == "tol2" and ptok == 1:
                seen |= set(want_s.reshape(-1).tolist())
    assert nq < 9 or len(seen) >= 3                                                       # the rule had something to decide
    # every element of every output is written: the C entry point on garbage-filled buffers
    rate, ptok = _rates(nq, 2)["budget"], 2
    P = -(-T // ptok)
    qa2 = torch.full((B, C, T), float("nan"), device=dev)
    en2 = torch.full((nq + 1, B * T), float("nan"), device=dev)
    nav2, nas2 = (torch.full((B, n), 0xAB, dtype=torch.uint8, device=dev) for n in (T, P))
    lib = _lib.lib()
    work = torch.empty(lib.mvq_dac_rvq_rate_workspace_bytes(B, C, T, nq) // 4, device=dev)
    rc = lib.mvq_dac_rvq_rate_f32(zd.data_ptr(), cd.data_ptr(), 0, cb.data_ptr(), ow.data_ptr(), ob.data_ptr(), qa2.data_ptr(),
                                  nav2.data_ptr(), nas2.data_ptr(), en2.data_ptr(), work.data_ptr(), work.numel() * 4, B, C, T, nq, K, 8,
                                  ptok, *rate.resolve(nq, ptok), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.mvq_last_error()
    want_q, want_v, want_s = _want(orc, q3, codes, zs, E, rate, ptok, B, T)
    assert np.array_equal(qa2.cpu().numpy(), want_q) and np.array_equal(nav2.cpu().numpy(), want_v)
    assert np.array_equal(nas2.cpu().numpy(), want_s) and np.array_equal(en2.cpu().numpy().reshape(E.shape), E)


def test_audio_rate_kernel_a_nan_token_and_the_first_stages_of_taller_codes(orc, dev):
    from multimodal_vqvae_compression_audio_tactile_amd import ops
    C, nq, K, B, T = 1024, 32, 1024, 3, 37
    q3, z, codes, _, zs, _ = _case(orc, C, nq, K, B, T)
    z = z.copy()
    z[1, 700, 20] = np.nan                                                                # a non-finite token takes all stages
    E = av.energies(z, zs)
    assert np.isnan(E[:, 1, 20]).all() and np.isfinite(np.delete(E.reshape(nq + 1, -1), 37 + 20, axis=1)).all()
    cb, ow, ob, zd, cd = _t(dev, *q3, z, codes)
    for rate in (Rate(tol2=TOL2), Rate(budget=8 * 16 + 3)):
        want_q, want_v, want_s = _want(orc, q3, codes, zs, E, rate, 2, B, T)
        qa, nav, nas, en = ops.dac_rvq_rate(zd, cd, cb, ow, ob, rate, 2, want_energy=True)
        assert np.array_equal(en.cpu().numpy().reshape(E.shape), E, equal_nan=True)
        assert np.array_equal(nas.cpu().numpy(), want_s) and np.array_equal(nav.cpu().numpy(), want_v)
        assert np.array_equal(qa.cpu().numpy(), want_q)
    assert rt.decide(E[:, 1], Rate(tol2=TOL2), 2)[10] == nq
    # na_use = 9 of the 32 rows, read in place
    E9 = E[:10]
    rate = Rate(min_books=2, tol2=TOL2)
    want_q, want_v, want_s = _want(orc, q3, codes, zs[:9], E9, rate, 2, B, T)
    qa, nav, nas = ops.dac_rvq_rate(zd, cd, cb, ow, ob, rate, 2, na_use=9)
    assert np.array_equal(nas.cpu().numpy(), want_s) and np.array_equal(qa.cpu().numpy(), want_q) and int(nas.max()) <= 9


def test_audio_rate_refusals_before_any_launch(dev):
    from multimodal_vqvae_compression_audio_tactile_amd import MvqError, ops
    cb, ow, ob = _t(dev, *av.quantiser(1, nq=4, K=37, C=128))
    z = torch.zeros(2, 128, 5, device=dev)
    codes = torch.zeros(2, 4, 5, dtype=torch.int64, device=dev)
    with pytest.raises(ValueError, match="does not divide"):
        ops.dac_rvq_rate(z, codes, cb, ow, ob, Rate(), 3)
    with pytest.raises(ValueError, match="min_books"):
        ops.dac_rvq_rate(z, codes, cb, ow, ob, Rate(min_books=5), 2)
    with pytest.raises(ValueError, match="budget"):
        ops.dac_rvq_rate(z, codes, cb, ow, ob, Rate(budget=33), 2)
    with pytest.raises(MvqError, match="na_use"):
        ops.dac_rvq_rate(z, codes, cb, ow, ob, Rate(), 2, na_use=5)
    with pytest.raises(ValueError, match="packets.Rate"):
        ops.dac_rvq_rate(z, codes, cb, ow, ob, (1, None, None), 2)
    with pytest.raises(MvqError):
        ops.dac_rvq_rate(z[:, :100].contiguous(), codes, cb, ow, ob, Rate(), 2)
    with pytest.raises(MvqError):
        ops.dac_rvq_rate(z, codes[:, :, :4].contiguous(), cb, ow, ob, Rate(), 2)


# ------------------------------------------------------------------------------------------------------ 3. through the model
def _net(dev, books=8, K=512, seed=7):
    if (books, K, seed) not in _NETS:
        import golden_inputs as gi
        from multimodal_vqvae_compression_audio_tactile_amd import build_proposed
        _NETS[(books, K, seed)] = build_proposed(gi.model_state(seed, books, K), rvq_books=books, rvq_embed=K, device=dev)
    return _NETS[(books, K, seed)]


# The seeded random weights exercise plumbing only: what these rates realise says nothing about quality.
RATES = {"full": (Rate(), Rate()), "tol2": (Rate(min_books=2, tol2=0.84), Rate(min_books=2, tol2=0.5)),
         "budget": (Rate(budget=27), Rate(budget=100))}


def _signals(dev, B, L):
    return synth.audio_segments(B, seed=L % 1000 + B, T=L).to(dev), synth.tactile_segments(B, seed=L % 1000 + B, T=L).to(dev)


def _per_token(sent, T, ptok=2):
    return torch.repeat_interleave(sent, ptok, dim=1)[:, :T].contiguous()


@pytest.mark.parametrize("name", list(RATES))
@pytest.mark.parametrize("Tlat", [16, 37])
@pytest.mark.parametrize("B", [1, 3, 9])
def test_closed_loop_on_both_streams_is_the_receivers(B, Tlat, name, dev):
    net, (rate, arate) = _net(dev), RATES[name]
    a, t = _signals(dev, B, 320 * Tlat)
    assert net._ar_one_call_mode(net.T_ENC(t), net.vq.stacked()) == ("staged" if B <= 8 else None)   # B = 9: the Python loop
    z_run, codes, idx, nb_sent, na_sent = net.encode_latents_with_indices(a, t, rate=rate, audio_rate=arate)
    assert z_run.shape == (B, 1024, Tlat) and codes.shape == (B, 32, Tlat) and idx.shape == (8, B, Tlat)
    assert na_sent.dtype == torch.uint8 and na_sent.shape == nb_sent.shape == (B, -(-Tlat // 2))
    lo_, hi_ = int(na_sent.min()), int(na_sent.max())
    assert arate.min_books <= lo_ and hi_ <= 32 and (name != "full" or lo_ == 32)
    if name == "budget":                                                  # 100 stages over 8 packets cannot come out equal
        assert len(set(na_sent[0, :8].tolist())) >= 2 and int(na_sent[0, :8].sum()) == 100
    nb_valid, na_valid = _per_token(nb_sent, Tlat), _per_token(na_sent, Tlat)
    assert torch.equal(z_run, net.decode_latents(codes, idx, nb_valid=nb_valid, na_valid=na_valid))
    # the audio latent the loop ran on is the layered look-up on the counts sent
    qa = net.A_QUANT.from_codes(codes, nq_valid=na_valid)[0]
    assert torch.equal(z_run, net.decode_latents(idx=idx, qa=qa, nb_valid=nb_valid))
    if name == "full":                                                    # everything sent: the tactile-only closed loop of section 18
        z1, c1, i1, s1 = net.encode_latents_with_indices(a, t, rate=rate)
        assert torch.equal(z1, z_run) and torch.equal(i1, idx) and torch.equal(c1, codes) and torch.equal(s1, nb_sent)


def test_audio_books_alone_equals_the_receiver_fed_the_first_rows(dev):
    net = _net(dev)
    a, t = _signals(dev, 3, 320 * 37)
    z_run, codes, idx, nb_sent, na_sent = net.encode_latents_with_indices(a, t, audio_books=9)
    assert bool((nb_sent == 8).all()) and bool((na_sent == 9).all())
    assert torch.equal(z_run, net.decode_latents(codes[:, :9], idx))
    assert torch.equal(z_run, net.decode_latents(codes, idx, na_valid=_per_token(na_sent, 37)))
    z32 = net.encode_latents_with_indices(a, t, rate=Rate())[0]
    assert not torch.equal(z32, z_run)                                    # nine stages are not thirty-two
    # thinned behind the sender's back: the receiver's z_run is NOT the sender's
    assert not torch.equal(z32, net.decode_latents(codes, idx, na_valid=torch.full((3, 37), 9, dtype=torch.uint8, device=dev)))


def test_receiver_na_valid_forms(dev):
    from multimodal_vqvae_compression_audio_tactile_amd import MvqError
    net = _net(dev)
    a, t = _signals(dev, 2, 320 * 37)
    _, codes, idx = net.encode_latents_with_indices(a, t)
    want = net.decode_latents(codes, idx)
    assert torch.equal(net.decode_latents(codes, idx, na_valid=None), want)
    assert torch.equal(net.decode_latents(codes, idx, na_valid=torch.full((2, 37), 32, dtype=torch.uint8, device=dev)), want)
    assert torch.equal(net.decode_latents(codes, idx, na_valid=torch.ones(2, 37, dtype=torch.bool, device=dev)), want)
    lostm = torch.zeros(2, 37, dtype=torch.bool, device=dev)
    lostm[:, 5:9] = True
    qa = net.A_QUANT.from_codes(codes)[0]
    qa[:, :, 5:9] = 0                                                     # a lost audio token is +0: silence to the predictor
    assert torch.equal(net.decode_latents(codes, idx, na_valid=~lostm), net.decode_latents(idx=idx, qa=qa))
    for bad in (torch.zeros(2, 36, dtype=torch.uint8, device=dev), torch.zeros(2, 37, dtype=torch.int32, device=dev)):
        with pytest.raises(MvqError, match="na_valid"):
            net.decode_latents(codes, idx, na_valid=bad)
    with pytest.raises(MvqError, match="na_valid"):
        net.decode_latents(idx=idx, qa=qa, na_valid=~lostm)


# ----------------------------------------------------------------------------------------------------- 4. the whole-item link
def _channel(pk, info, seed):
    """A seeded lossy channel over one item's packets: drops, thinning, a reversal and a duplicate -> (what arrives, the count
    of each packet as the receiver will see it)."""
    r = np.random.default_rng(seed)
    recv = np.zeros(info.P, np.int64)
    out = []
    for s, p in enumerate(pk):
        u = r.uniform()
        if u < 0.25:
            continue                                                                      # dropped
        if u < 0.55 and p[8] > 1:
            p = packets.thin(p, int(r.integers(1, p[8])), info)                           # thinned by a relay
        recv[s] = p[8]
        out.append(p)
    out = out[::-1]
    if out:
        out.append(out[0])                                                                # a duplicate
    return out, recv


@pytest.mark.parametrize("name", list(RATES))
def test_whole_item_link(name, dev):
    net, (rate, arate) = _net(dev), RATES[name]
    B, Tlat = 3, 37
    a, t = _signals(dev, B, 320 * Tlat)
    z_run, codes, idx, nb_sent, na_sent = net.encode_latents_with_indices(a, t, rate=rate, audio_rate=arate)
    infos, pk, ainfos, apk = net.compress_packets_av(a, t, rate=rate, audio_rate=arate)
    info, ainfo = infos[0], ainfos[0]
    assert info == StreamInfo(512, 8, Tlat, 2) and ainfo == StreamInfo(1024, 32, Tlat, 2)
    assert all(i == info for i in infos) and all(i == ainfo for i in ainfos)
    codes_h, idx_h, nas, nbs = codes.cpu().numpy(), idx.cpu().numpy(), na_sent.cpu().numpy(), nb_sent.cpu().numpy()
    for b in range(B):
        assert apk[b] == packets.frame(packets.pack_bodies(codes_h[b], ainfo), ainfo, nb_sent=nas[b])
        assert pk[b] == packets.frame(packets.pack_bodies(idx_h[:, b], info), info, nb_sent=nbs[b])
    if name == "full":                                                    # audio sent in full: the tactile packets of section 18
        assert pk == net.compress_packets(a, t, rate=rate)[1]
    # nothing lost: the sender's own z_run, decoded
    y, lost, alost = net.decompress_packets_av(infos, pk, ainfos, apk)
    assert torch.equal(y, net.T_DEC(z_run)) and not bool(lost.any()) and not bool(alost.any())
    assert lost.shape == alost.shape == (B, Tlat) and alost.dtype == torch.bool
    # both streams over a lossy channel: the restatement's arrays through decode
    rx, arx, nbr, nar = [], [], [], []
    for b in range(B):
        got, recv = _channel(pk[b], info, 10 * b + 1)
        rx.append(got); nbr.append(recv)
        got, recv = _channel(apk[b], ainfo, 10 * b + 2)
        arx.append(got); nar.append(recv)
    hi, hv, hc, ha = [], [], [], []
    for b in range(B):
        bodies, recv = packets.gather(rx[b], info)
        assert np.array_equal(recv, nbr[b])
        i_b, v_b = packets.unpack_bodies(bodies, recv, info)
        bodies, recv = packets.gather(arx[b], ainfo)
        assert np.array_equal(recv, nar[b])
        c_b, a_b = packets.unpack_bodies(bodies, recv, ainfo)
        hi.append(i_b); hv.append(v_b); hc.append(c_b); ha.append(a_b)
    idx_r, nbv, codes_r, nav = _t(dev, np.stack(hi, axis=1), np.stack(hv).astype(np.uint8), np.stack(hc, axis=0), np.stack(ha).astype(np.uint8))
    assert int((nav == 0).sum()) > 0 and int((nbv == 0).sum()) > 0 and len(set(nav.reshape(-1).tolist())) >= 3
    for conceal in ("predict", "zero"):
        y, lost, alost = net.decompress_packets_av(infos, rx, ainfos, arx, conceal=conceal)
        assert torch.equal(y, net.decode(codes_r, idx_r, nb_valid=nbv, na_valid=nav, conceal=conceal)), conceal
        assert torch.equal(lost, nbv == 0) and torch.equal(alost, nav == 0)
    if name == "tol2":
        from multimodal_vqvae_compression_audio_tactile_amd import AllPredPLC
        plc = AllPredPLC(net.A_ENC, net.A_QUANT, net.T_ENC, net.T_DEC, c_lat=1024)        # seeded, on the receiver's own backbones
        head = synth.proposed_head_state(23, rvq_books=1, rvq_embed=128)
        plc.predict.load_state_dict({k[len("predict."):]: v for k, v in head.items() if k.startswith("predict.")}, strict=False)
        plc = plc.to(dev).eval()
        y, _, _ = net.decompress_packets_av(infos, rx, ainfos, arx, conceal="plc", plc=plc)
        assert torch.equal(y, net.decode(codes_r, idx_r, nb_valid=nbv, na_valid=nav, conceal="plc", plc=plc))
        assert not torch.equal(y, net.decode(codes_r, idx_r, nb_valid=nbv, na_valid=nav))


def test_compress_packets_av_with_nine_stages_and_other_packet_sizes(dev):
    net = _net(dev)
    B, Tlat = 1, 16
    a, t = _signals(dev, B, 320 * Tlat)
    for ptok in (1, 16):
        arate = Rate(min_books=2, budget=(16 // ptok) * 5)
        z_run, codes, idx, nb_sent, na_sent = net.encode_latents_with_indices(a, t, packet_tok=ptok, audio_books=9, audio_rate=arate)
        infos, pk, ainfos, apk = net.compress_packets_av(a, t, packet_tok=ptok, audio_books=9, audio_rate=arate)
        ainfo = ainfos[0]
        assert ainfo == StreamInfo(1024, 9, Tlat, ptok) and int(na_sent.sum()) == (16 // ptok) * 5
        assert apk[0] == packets.frame(packets.pack_bodies(codes[0, :9].cpu().numpy(), ainfo), ainfo, nb_sent=na_sent[0].cpu().numpy())
        y, _, alost = net.decompress_packets_av(infos, pk, ainfos, apk)
        assert torch.equal(y, net.T_DEC(z_run)) and not bool(alost.any())


# ------------------------------------------------------------------------------------------------------------ 5. streaming
def _run_sender(tx, a, t, pushes):
    out, pos = [], 0
    for m in pushes:
        out.append(tx.push(a[..., pos:pos + 320 * m], t[..., pos:pos + 320 * m]))
        pos += 320 * m
    pk, apk, info, ainfo = tx.finish(a[..., pos:], t[..., pos:]) if pos < a.shape[-1] else tx.finish()
    out.append((pk, apk))
    return out, info, ainfo


@pytest.mark.parametrize("L", [24000, 12663])
@pytest.mark.parametrize("B", [1, 3])
def test_stream_sender_audio_packets_equals_compress_packets_av(B, L, dev):
    net = _net(dev)
    rate, arate = RATES["tol2" if L == 24000 else "budget"]
    a, t = _signals(dev, B, L)
    infos, pk, ainfos, apk = net.compress_packets_av(a, t, rate=rate, audio_rate=arate)
    for pattern in (16, "mixed", 1):
        tx = net.stream_sender(batch=B, rate=rate, audio="packets", audio_rate=arate)
        out, info, ainfo = _run_sender(tx, a, t, sn.split_pushes(L, pattern, seed=L + B))
        assert info == infos[0] and ainfo == ainfos[0] and tx.finished
        for b in range(B):                                                # byte for byte, in order, both streams
            assert sum((step[0][b] for step in out), []) == pk[b], (pattern, b)
            assert sum((step[1][b] for step in out), []) == apk[b], (pattern, b)


def test_stream_sender_audio_packets_graph_equals_eager(dev):
    net = _net(dev)
    rate, arate = RATES["tol2"]
    L = 320 * 96
    a, t = _signals(dev, 1, L)
    kw = dict(batch=1, rate=rate, audio="packets", audio_rate=arate)
    eager, info_e, ainfo_e = _run_sender(net.stream_sender(**kw), a, t, [16] * 6)
    txg = net.stream_sender(graph=True, **kw)
    graphed, info_g, ainfo_g = _run_sender(txg, a, t, [16] * 6)
    assert txg._g is not None and isinstance(txg._g[0], torch.cuda.CUDAGraph) and (info_e, ainfo_e) == (info_g, ainfo_g)
    assert eager == graphed
    infos, pk, ainfos, apk = net.compress_packets_av(a, t, rate=rate, audio_rate=arate)
    assert sum((step[0][0] for step in graphed), []) == pk[0] and sum((step[1][0] for step in graphed), []) == apk[0]


@pytest.mark.parametrize("graph", [False, True])
def test_stream_sender_into_stream_receiver_equals_the_whole_item_link(graph, dev):
    net = _net(dev)
    rate, arate = RATES["tol2"]
    B, L = 3, 320 * 91                                                    # five whole chunks (the graph replays) and a tail of 11 tokens
    a, t = _signals(dev, B, L)
    tx = net.stream_sender(batch=B, rate=rate, audio="packets", audio_rate=arate)
    out, info, ainfo = _run_sender(tx, a, t, sn.split_pushes(L, "mixed", seed=3))
    pk = [sum((step[0][b] for step in out), []) for b in range(B)]
    apk = [sum((step[1][b] for step in out), []) for b in range(B)]
    rx_pk = [_channel(pk[b], info, 10 * b + 1)[0] for b in range(B)]
    rx_apk = [_channel(apk[b], ainfo, 10 * b + 2)[0] for b in range(B)]
    for conceal in ("predict", "zero"):
        want, lost, alost = net.decompress_packets_av([info] * B, rx_pk, [ainfo] * B, rx_apk, conceal=conceal)
        assert bool(lost.any()) and bool(alost.any())
        rx = net.stream_receiver(512, 8, batch=B, conceal=conceal, graph=graph, audio=(1024, 32))
        seq = lambda p: int.from_bytes(bytes(p)[3:7], "little")
        ys = []
        for c in range(info.T // 16):
            pick = lambda lists: [[p for p in lists[b] if 8 * c <= seq(p) < 8 * c + 8] for b in range(B)]
            ys.append(rx.push(pick(rx_pk), audio_packets=pick(rx_apk)).clone())
        tail = lambda lists: [[p for p in lists[b] if seq(p) >= 8 * (info.T // 16)] for b in range(B)]
        ys.append(rx.finish(tail(rx_pk), tail(rx_apk), tokens=info.T % 16))
        got = torch.cat(ys, dim=-1)
        assert got.shape == want.shape and torch.equal(got, want), conceal
        if graph:
            assert rx._g is not None and isinstance(rx._g[0], torch.cuda.CUDAGraph)


def test_streaming_refusals(dev):
    from multimodal_vqvae_compression_audio_tactile_amd import ops
    net = _net(dev)
    with pytest.raises(ValueError, match="audio"):
        net.stream_sender(audio="bits")
    with pytest.raises(ValueError, match="audio"):
        net.stream_sender(audio_rate=Rate())                              # audio_rate without audio="packets"
    with pytest.raises(ValueError, match="packets.Rate"):
        net.stream_sender(audio="packets", audio_rate=0.5)
    with pytest.raises(ValueError, match="audio_books"):
        net.stream_sender(audio="packets", audio_books=40)
    with pytest.raises(ValueError, match="audio"):
        net.stream_receiver(512, 8, audio=(512, 32))
    with pytest.raises(ValueError, match="audio"):
        net.stream_receiver(512, 8, audio=(1024, 33))
    with ops.arith("f16x3"):
        with pytest.raises(ValueError, match="arithmetic"):
            net.stream_sender(audio="packets")
        with pytest.raises(ValueError, match="arithmetic"):
            net.stream_receiver(512, 8, audio=(1024, 32))
    for make in (net.stream_sender_pool, lambda **kw: net.stream_receiver_pool(512, 8, **kw)):   # the pools take none of this
        with pytest.raises(TypeError):
            make(audio="packets")
    rx = net.stream_receiver(512, 8, audio=(1024, 32))
    with pytest.raises(ValueError, match="tokens"):
        rx.finish([[]], [[]])
    with pytest.raises(ValueError, match="tokens"):                               # tokens= without audio packets
        net.stream_receiver(512, 8).finish(tokens=3)
    with pytest.raises(ValueError, match="audio_packets"):
        net.stream_receiver(512, 8).push([[]], audio_packets=[[]])


# ------------------------------------------------------------------------------------------------------------- 6. refusals
def test_av_refusals_on_the_device_model(dev):
    from multimodal_vqvae_compression_audio_tactile_amd import ops
    net = _net(dev)
    a, t = _signals(dev, 1, 320 * 16)
    for call in (lambda **kw: net.encode_latents_with_indices(a, t, **kw), lambda **kw: net.compress_packets_av(a, t, **kw)):
        with pytest.raises(ValueError, match="packets.Rate"):
            call(audio_rate=0.5)
        with pytest.raises(ValueError, match="audio_books"):
            call(audio_books=33)
        with pytest.raises(ValueError, match="audio_books"):
            call(audio_books=0)
        with ops.arith("f16x3"):
            with pytest.raises(ValueError, match="arithmetic"):
                call(audio_rate=Rate())
    infos, pk, ainfos, apk = net.compress_packets_av(a, t)
    with pytest.raises(ValueError, match="audio"):
        net.decompress_packets_av(infos, pk, [StreamInfo(512, 32, 16, 2)], apk)
    with pytest.raises(ValueError, match="audio"):
        net.decompress_packets_av(infos, pk, [StreamInfo(1024, 33, 16, 2)], apk)
    with pytest.raises(ValueError, match="advance together"):
        net.decompress_packets_av(infos, pk, [StreamInfo(1024, 32, 15, 2)], apk)
