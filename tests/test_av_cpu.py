"""CPU: the audio transport restated in numpy (tests/av_oracle.py) and everything about it that needs no device.

  * the restated layered from_codes against receiver_oracle.from_codes's arithmetic on the prefix;
  * the restated energy chain (its fixed summation order) and the decision on audio-sized tables;
  * audio packets in the existing format: frame with per-packet counts against thin, the gather / unpack round trip;
  * THE DESIGN CLAIM: with counts on both streams the closed loop's z_run equals the receiver's; thinning behind the sender does not;
  * the condition the GPU tests rely on: the kernel-level inputs make the rule decide something;
  * the new symbols are exported and refuse bad arguments; the Python surface refuses before any launch."""
import inspect

import numpy as np
import pytest
import torch

import av_oracle as av
import rate_oracle as rt
from multimodal_vqvae_compression_audio_tactile_amd import packets, synth
from multimodal_vqvae_compression_audio_tactile_amd.packets import Rate, StreamInfo

f32 = np.float32


@pytest.fixture(scope="module")
def q128():
    return av.quantiser(5, nq=9, K=37, C=128)


# ---------------------------------------------------------------------------------------------------- 1. layered from_codes
@pytest.mark.parametrize("B,T", [(3, 37), (2, 5)])
def test_layered_from_codes_is_from_codes_of_the_prefix(B, T, orc, q128):
    cb, ow, ob = q128
    r = np.random.default_rng(B + T)
    codes = r.integers(-2, 40, size=(B, 9, T))                                            # some out of range: clamped
    count = r.integers(0, 13, size=(B, T))                                                # 0 and values above nq
    count[0, 0], count[0, 1] = 0, 255
    got = av.from_codes_layers(orc, cb, ow, ob, codes, count)
    for m in range(0, 10):
        cols = np.minimum(count, 9) == m
        if m == 0:
            want = np.zeros_like(got)
        else:                                                                             # receiver_oracle.from_codes's loop on codes[:, :m]
            want = None
            for zi in av.stages(orc, cb, ow, ob, codes[:, :m]):
                want = np.zeros_like(zi) + zi if want is None else want + zi
        assert np.array_equal(got.transpose(0, 2, 1)[cols], want.transpose(0, 2, 1)[cols]), m
    zero = got.transpose(0, 2, 1)[count == 0]
    assert zero.size and not np.signbit(zero).any() and np.all(zero == 0)                 # +0, no bias


def test_layered_from_codes_on_model_weights_is_receiver_oracles(orc):
    import receiver_oracle as ro
    sd = {k: v.numpy() for k, v in synth.proposed_model_state(7, rvq_books=3, rvq_embed=128).items() if k.startswith("A_QUANT.")}
    q3 = av.quantiser_of(orc, sd)
    assert q3[0].shape == (32, 1024, 8) and q3[1].shape == (32, 1024, 8) and q3[2].shape == (32, 1024)
    codes = np.random.default_rng(1).integers(0, 1024, size=(1, 32, 6))
    for m in (1, 9, 32):
        want, _ = ro.from_codes(orc, sd, codes[:, :m])
        assert np.array_equal(av.from_codes_layers(orc, *q3, codes, np.full((1, 6), m)), want)


# ------------------------------------------------------------------------------------------------- 2. energies and decision
def test_energy_sum_order_is_the_documented_one():
    r = np.random.default_rng(0)
    p = r.uniform(0, 1, size=(1, 128, 2)).astype(f32)
    E = av.energy_sum(p)
    for t in range(2):
        e = f32(0)
        for s in range(2):
            P = f32(0)
            for g in range(16):
                tt = f32(0)
                for u in range(4):
                    tt = f32(tt + p[0, 64 * s + 16 * u + g, t])
                P = f32(P + tt)
            e = f32(e + P)
        assert E[0, t] == e
    # position independent: a token's energy does not change with what stands around it
    assert np.array_equal(av.energy_sum(np.concatenate([p, p[..., :1]], axis=-1))[:, 2], E[:, 0])


def test_energy_chain_is_the_running_sum(orc, q128):
    cb, ow, ob = q128
    z, codes, m_t = av.layered_inputs(orc, cb, ow, ob, 2, 5, 9, seed=3)
    zs = av.stages(orc, cb, ow, ob, codes)
    E = av.energies(z, zs)
    assert E.shape == (10, 2, 5) and E.dtype == f32
    S = np.zeros_like(z)
    for m in range(10):
        d = z - S
        assert np.array_equal(E[m], av.energy_sum(d * d))
        assert np.array_equal(S, av.from_codes_layers(orc, cb, ow, ob, codes, np.full((2, 5), m)))   # S_m IS the layered look-up
        if m < 9:
            S = S + zs[m]
    # the energy is smallest (noise only) at the count the token was built from
    assert np.array_equal(E.argmin(axis=0), m_t)


@pytest.mark.parametrize("ptok", [1, 2, 16])
def test_decision_on_audio_tables(ptok):
    na, pc = 32, 16 // ptok
    r = np.random.default_rng(ptok)
    for T in (16, 37, 5):
        steps = r.uniform(0.05, 1.0, size=(na + 1, T)).astype(f32)
        E = np.ascontiguousarray(np.cumsum(steps[::-1], axis=0)[::-1]).astype(f32)
        P = -(-T // ptok)
        assert np.array_equal(rt.decide(E, Rate(), ptok), np.full(P, na))
        for mb in (1, 9):
            got = rt.decide(E, Rate(min_books=mb, tol2=0.3), ptok)
            assert got.min() >= mb and got.max() <= na                                    # min_books is respected
            for budget in (pc * mb, pc * mb + 5, pc * na):
                got = rt.decide(E, Rate(min_books=mb, budget=budget), ptok)
                assert got.min() >= mb and got.max() <= na
                for g0 in range(0, P, pc):                                                # spent exactly; the tail-group formula
                    g = min(pc, P - g0)
                    assert got[g0:g0 + pc].sum() == max(g * mb, budget * g // pc)
    E = np.tile(np.arange(na, -1, -1, dtype=f32)[:, None], (1, 16))                       # every gain ties: the lowest packet wins
    assert rt.decide(E, Rate(budget=8 + 3), 2).tolist() == [4, 1, 1, 1, 1, 1, 1, 1]
    En = E.copy()
    En[:, 5] = np.nan                                                                     # a NaN token takes all stages
    got = rt.decide(En, Rate(tol2=0.99), 2)
    assert got[2] == na and got[0] == 1


# --------------------------------------------------------------------------------------------------------- 3. audio packets
@pytest.mark.parametrize("nb", [32, 9])
@pytest.mark.parametrize("ptok", [1, 2, 16])
@pytest.mark.parametrize("T", [16, 37, 5])
def test_audio_packets_use_the_existing_format(nb, ptok, T):
    info = StreamInfo(av.K_AUDIO, nb, T, ptok)
    r = np.random.default_rng(nb + ptok + T)
    codes = r.integers(0, av.K_AUDIO, size=(nb, T))
    bodies = packets.pack_bodies(codes, info)
    whole = packets.frame(bodies, info)
    counts = r.integers(1, nb + 1, size=info.P)
    got = packets.frame(bodies, info, nb_sent=counts)
    assert got == [packets.thin(whole[p], int(counts[p]), info) for p in range(info.P)]
    g_bodies, g_recv = packets.gather(got, info)
    assert np.array_equal(g_recv, counts)
    back, nav = packets.unpack_bodies(g_bodies, g_recv, info)
    assert np.array_equal(nav, rt.expand(counts, T, ptok))
    assert np.array_equal(back, np.where(np.arange(nb)[:, None] < nav[None, :], codes, 0))
    assert packets.sent_bits(counts, info) == 8 * sum(len(p) for p in got)


def test_full_audio_stream_is_24_kbps():
    assert packets.sent_kbps(32, StreamInfo(av.K_AUDIO, 32, 75, 2), headers=False) == pytest.approx(24.0, rel=0.01)


# ----------------------------------------------------------------------------------------------------- 4. the design claim
@pytest.fixture(scope="module")
def head_sd():
    return {k: v.numpy() for k, v in synth.proposed_head_state(17, rvq_books=3, rvq_embed=128).items()}


@pytest.mark.parametrize("B,Tlat", [(2, 37), (1, 16)])
def test_closed_loop_on_both_streams_equals_the_receiver(B, Tlat, orc, head_sd):
    import lossy_oracle as lo
    q3 = av.quantiser(11, nq=9, K=64, C=1024)
    za, codes, _ = av.layered_inputs(orc, *q3, B, Tlat, 9, seed=Tlat, noise=0.05)
    zt = (0.5 * np.random.default_rng(Tlat + 1).standard_normal((B, 1024, Tlat))).astype(f32)
    seen = set()
    for rate, arate in ((Rate(), Rate()), (Rate(tol2=0.9), Rate(tol2=0.05)), (Rate(budget=14), Rate(min_books=2, budget=40)),
                        (Rate(min_books=2, tol2=0.5), Rate(tol2=1e-4))):
        z_run, idx, nb_valid, nb_sent, na_valid, na_sent, qa = av.closed_loop_av(orc, head_sd, q3, za, codes, zt, rate, arate)
        assert na_valid.shape == (B, Tlat) and na_sent.shape == (B, -(-Tlat // 2))
        assert np.array_equal(na_valid, rt.expand(na_sent, Tlat, 2))
        assert np.array_equal(z_run, av.receiver_av(orc, head_sd, q3, codes, idx, nb_valid, na_valid))
        seen |= set(na_sent.reshape(-1).tolist())
    assert len(seen) >= 3
    # the same codes thinned BEHIND the sender: it ran on all stages, the receiver gets three
    z_open, idx, nb_valid, _, _, _, _ = av.closed_loop_av(orc, head_sd, q3, za, codes, zt, Rate(), Rate())
    thin = np.full((B, Tlat), 3, np.uint8)
    assert not np.array_equal(z_open, av.receiver_av(orc, head_sd, q3, codes, idx, nb_valid, thin))
    # a lost audio token is +0: the predictor attends over it as over silence
    lost = np.full((B, Tlat), 9, np.uint8)
    lost[:, 3] = 0
    qa = av.from_codes_layers(orc, *q3, codes, lost)
    assert np.all(qa[:, :, 3] == 0) and np.array_equal(av.receiver_av(orc, head_sd, q3, codes, idx, nb_valid, lost),
                                                       lo.lossy_loop(orc, head_sd, qa, idx, nb_valid))


# ------------------------------------------------------------------------- 5. the condition the GPU tests rely on
KERNEL_SHAPES = [(128, 9, 37, 3, 37), (1024, 32, 1024, 1, 16), (128, 1, 37, 2, 5), (1024, 9, 1024, 2, 5)]   # C, nq, K, B, T
TOL2 = 1e-3


@pytest.mark.parametrize("C,nq,K,B,T", KERNEL_SHAPES)
def test_kernel_level_inputs_make_the_rule_decide(C, nq, K, B, T, orc):
    q3 = av.quantiser(C + nq, nq=nq, K=K, C=C)
    z, codes, m_t = av.layered_inputs(orc, *q3, B, T, nq, seed=C + T)
    _, _, sent, E = av.rate_audio(orc, *q3, z, codes, Rate(tol2=TOL2), 1)
    if nq >= 9:
        assert len(set(sent.reshape(-1).tolist())) >= 3
        pc_budget = 16 * max(1, nq // 2)
        _, _, sb, _ = av.rate_audio(orc, *q3, z, codes, Rate(budget=pc_budget), 1)
        assert len(set(sb[0].tolist())) >= 2
    else:
        assert set(sent.reshape(-1).tolist()) <= {1}


# --------------------------------------------------------------------------------------------------------- 6. refusals, ABI
def test_av_entry_points_are_exported_and_check_their_arguments():
    from multimodal_vqvae_compression_audio_tactile_amd import ProposedEval, _lib, ops, torch_ops
    from multimodal_vqvae_compression_audio_tactile_amd.dac import ResidualVectorQuantize
    lib = _lib.lib()
    for n in ("mvq_dac_rvq_from_codes_layers_f32", "mvq_dac_rvq_rate_f32", "mvq_dac_rvq_rate_workspace_bytes"):
        assert n in _lib.EXPORTS and hasattr(lib, n), n
    assert lib.mvq_abi_version() == 3
    assert "nq_valid" in inspect.signature(ops.dac_rvq_from_codes).parameters
    assert "nq_valid" in inspect.signature(ResidualVectorQuantize.from_codes).parameters
    assert "dac_rvq_from_codes_layers" in torch_ops.REGISTERED
    for fn in (ProposedEval.decode_latents, ProposedEval.decode):
        assert "na_valid" in inspect.signature(fn).parameters, fn
    for name in ("audio_books", "audio_rate"):
        assert name in inspect.signature(ProposedEval.encode_latents_with_indices).parameters
        assert name in inspect.signature(ProposedEval.compress_packets_av).parameters
        assert name not in inspect.signature(ProposedEval.compress_packets).parameters   # the old pair keeps its signature
    assert lib.mvq_dac_rvq_rate_workspace_bytes(2, 1024, 37, 32) == 16 * 33 * 74 * 4
    from multimodal_vqvae_compression_audio_tactile_amd import StreamReceiver, StreamSender
    for fn, names in ((StreamSender.__init__, ("audio", "audio_books", "audio_rate")), (ProposedEval.stream_sender, ("audio", "audio_rate")),
                      (StreamReceiver.__init__, ("audio",)), (ProposedEval.stream_receiver, ("audio",))):
        for name in names:
            assert name in inspect.signature(fn).parameters, (fn, name)
    for fn in (ProposedEval.stream_sender_pool, ProposedEval.stream_receiver_pool):      # the pools are out of scope
        assert "audio" not in inspect.signature(fn).parameters

    def rate(batch=1, c=1024, t=16, na=32, k=1024, dc=8, ptok=2, mb=1, mode=0, tol2=0.0, budget=0):
        return lib.mvq_dac_rvq_rate_f32(None, None, 0, None, None, None, None, None, None, None, None, 0, batch, c, t, na, k, dc, ptok, mb,
                                        mode, tol2, budget, None)
    assert rate() == -1 and b"null" in lib.mvq_last_error()                              # a good shape gets as far as the tensors
    assert rate(batch=0) == 0 and rate(t=0) == 0
    for kw in (dict(batch=-1), dict(t=-1), dict(c=0), dict(na=0), dict(k=0), dict(ptok=0), dict(ptok=3), dict(mb=0), dict(mb=33),
               dict(mode=3), dict(mode=1, tol2=0.0), dict(mode=1, tol2=float("nan")), dict(mode=2, budget=7), dict(mode=2, budget=257)):
        assert rate(**kw) == -1, kw
    for kw in (dict(c=1000), dict(dc=4), dict(na=33)):
        assert rate(**kw) == -2, kw
    assert rate(ptok=3) == -1 and lib.mvq_last_error().startswith(b"dac_rvq_rate:") and b"divide" in lib.mvq_last_error()

    def layers(batch=1, c=1024, t=16, nq=32, k=1024, dc=8, sb=1):
        return lib.mvq_dac_rvq_from_codes_layers_f32(None, sb, None, None, None, None, None, None, batch, c, t, nq, k, dc, None)
    assert layers() == -1 and layers(batch=0, sb=0) == 0
    for kw in (dict(c=1000), dict(dc=4), dict(nq=33), dict(nq=0), dict(k=0), dict(batch=-1)):
        assert layers(**kw) == -1, kw


def test_torch_operator_has_a_shape_only_fake():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from multimodal_vqvae_compression_audio_tactile_amd import torch_ops  # noqa: F401
    with FakeTensorMode():
        zq, zp = torch.ops.mi355x_vqvae.dac_rvq_from_codes_layers(
            torch.empty(2, 9, 37, dtype=torch.int64), torch.empty(9, 1024, 8), torch.empty(9, 128, 8), torch.empty(9, 128),
            torch.empty(2, 37, dtype=torch.uint8))
    assert tuple(zq.shape) == (2, 128, 37) and tuple(zp.shape) == (2, 72, 37)


@pytest.fixture(scope="module")
def cpu_net():
    from multimodal_vqvae_compression_audio_tactile_amd import build_proposed
    return build_proposed(None, rvq_books=2, rvq_embed=128, device="cpu")


def test_av_refusals_come_before_any_launch(cpu_net):
    """On a CPU-resident model nothing can have been launched: the checks come first."""
    from multimodal_vqvae_compression_audio_tactile_amd import ops
    net = cpu_net
    x = torch.zeros(1, 1, 5120)
    for call in (lambda **kw: net.encode_latents_with_indices(x, x, **kw), lambda **kw: net.compress_packets_av(x, x, **kw)):
        with pytest.raises(ValueError, match="packets.Rate"):
            call(audio_rate=(1, None, None))
        with pytest.raises(ValueError, match="audio_books"):
            call(audio_books=0)
        with pytest.raises(ValueError, match="audio_books"):
            call(audio_books=33)
        with pytest.raises(ValueError, match="min_books"):
            call(audio_books=9, audio_rate=Rate(min_books=10))
        with pytest.raises(ValueError, match="budget"):
            call(audio_rate=Rate(budget=7))
        with pytest.raises(ValueError, match="does not divide"):
            call(audio_rate=Rate(), packet_tok=3)
        with pytest.raises(ValueError, match="min_books"):                                # the tactile rate is still checked
            call(audio_rate=Rate(), rate=Rate(min_books=3))
        with ops.arith("f16x3"):
            with pytest.raises(ValueError, match="arithmetic"):
                call(audio_rate=Rate())
    with pytest.raises(ValueError, match="audio"):
        net.stream_sender(audio="bits")
    with pytest.raises(ValueError, match="audio"):
        net.stream_sender(audio_rate=Rate())                                              # audio_rate without audio="packets"
    with pytest.raises(ValueError, match="packets.Rate"):
        net.stream_sender(audio="packets", audio_rate=0.5)
    with pytest.raises(ValueError, match="audio_books"):
        net.stream_sender(audio="packets", audio_books=40)
    with pytest.raises(ValueError, match="audio"):
        net.stream_receiver(128, 2, audio=(512, 32))
    with ops.arith("f16x3"):
        with pytest.raises(ValueError, match="arithmetic"):
            net.stream_sender(audio="packets")
    tx = net.stream_sender(audio="packets", audio_books=9, audio_rate=Rate(budget=40))
    assert tx.rate == Rate() and tx.audio_rate == Rate(budget=40) and tx.na == 9 and net.stream_sender().audio_packets is False
    info = StreamInfo(128, 2, 16, 2)
    with pytest.raises(ValueError, match="audio"):                                        # an audio stream whose K is not the quantiser's
        net.decompress_packets_av([info], [[]], [StreamInfo(512, 32, 16, 2)], [[]])
    with pytest.raises(ValueError, match="packet_tok"):
        net.decompress_packets_av([info], [[]], [StreamInfo(1024, 32, 16, 4)], [[]])
