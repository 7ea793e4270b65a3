"""CPU: closed-loop sender rate control restated in numpy (tests/rate_oracle.py) and everything about it that needs no device.

  * the restated residual chain is the search's own (oracle.rvq_ema_forward(return_residual=True));
  * the decision rule's properties: min_books, the budget spent exactly (tail groups too), ties to the lowest packet, a NaN token
    takes all books;
  * packets.Rate's validation, frame() with one count per packet against thin(), the realised-rate arithmetic;
  * THE DESIGN CLAIM: the closed loop's z_run equals the receiver's restatement (per-chunk loop and two passes) on the same
    indices, counts and audio latent, bit for bit;
  * refusals come before any launch; the new symbols are exported and refuse bad shapes."""
import ctypes

import numpy as np
import pytest
import torch

import lossy_oracle as lo
import rate_oracle as rt
import receiver_oracle as ro
from multimodal_vqvae_compression_audio_tactile_amd import packets, synth
from multimodal_vqvae_compression_audio_tactile_amd.packets import Rate, StreamInfo


# ------------------------------------------------------------------------------------------------------------ 1. arithmetic
@pytest.mark.parametrize("nb,K", [(8, 512), (3, 128), (10, 128)])
def test_restated_residual_is_the_searchs(nb, K, orc):
    sd = {k: v.numpy() for k, v in synth.proposed_head_state(175, rvq_books=nb, rvq_embed=K).items()}
    rD = rt.real_rD(orc, sd, 3, 16, seed=nb)
    books = ro.books_of(sd)
    _, idx, res = orc.rvq_ema_forward(rD, books, None, return_residual=True)
    E, r = rt.energies(rD, books, idx.reshape(nb, 3, 16))
    assert np.array_equal(r.reshape(-1, 96), res)
    assert E.shape == (nb + 1, 3, 16) and E.dtype == np.float32 and np.all(E[1:] < E[:-1])   # every book removes energy here
    # the chain is the sequential fp32 one, multiply and add rounded separately
    tok = rD[1, :, 7]
    e = np.float32(0.0)
    for d in range(96):
        e = np.float32(e + np.float32(tok[d] * tok[d]))
    assert E[0, 1, 7] == e


# --------------------------------------------------------------------------------------------------------------- 2. decide
def _E(nb, T, seed):
    """A decreasing energy table [nb + 1, T]."""
    r = np.random.default_rng(seed)
    steps = r.uniform(0.05, 1.0, size=(nb + 1, T)).astype(np.float32)
    return np.ascontiguousarray(np.cumsum(steps[::-1], axis=0)[::-1]).astype(np.float32)


@pytest.mark.parametrize("ptok", [1, 2, 4, 16])
def test_decide_respects_min_books_and_spends_the_budget(ptok):
    nb, pc = 8, 16 // ptok
    for T in (16, 37, 5, 33):
        E = _E(nb, T, T + ptok)
        P = -(-T // ptok)
        assert np.array_equal(rt.decide(E, Rate(), ptok), np.full(P, nb))
        for mb in (1, 3, 8):
            got = rt.decide(E, Rate(min_books=mb, tol2=0.5), ptok)
            assert got.shape == (P,) and got.min() >= mb and got.max() <= nb
            for p in range(P):                                                          # the max over the packet of the per-token need
                need = [next((m for m in range(mb, nb + 1) if E[m, j] <= np.float32(0.5) * E[0, j]), nb)
                        for j in range(p * ptok, min(T, (p + 1) * ptok))]
                assert got[p] == max(need)
            for budget in sorted({pc * mb, min(pc * mb + 1, pc * nb), pc * (mb + nb) // 2, pc * nb}):
                got = rt.decide(E, Rate(min_books=mb, budget=budget), ptok)
                assert got.min() >= mb and got.max() <= nb
                for g0 in range(0, P, pc):
                    g = min(pc, P - g0)
                    assert got[g0:g0 + pc].sum() == max(g * mb, budget * g // pc), (T, mb, budget, g0)


def test_decide_ties_go_to_the_lowest_packet_and_nan_takes_all_books():
    nb = 4
    E = np.tile(np.arange(nb, -1, -1, dtype=np.float32)[:, None], (1, 16))              # every token, every book: gain 1
    assert rt.decide(E, Rate(budget=8 + 3), 2).tolist() == [4, 1, 1, 1, 1, 1, 1, 1]      # its next book ties again: packet 0 until it is full
    assert rt.decide(E, Rate(budget=8 + 7), 2).tolist() == [4, 4, 2, 1, 1, 1, 1, 1]
    E2 = E.copy()
    E2[:, 6:8] *= 4                                                                      # packet 3 is loud: it is served first
    assert rt.decide(E2, Rate(budget=8 + 4), 2).tolist() == [2, 1, 1, 4, 1, 1, 1, 1]
    En = E.copy()
    En[:, 5] = np.nan                                                                    # a NaN token, constant quality: all books
    got = rt.decide(En, Rate(tol2=0.9), 2)
    assert got[2] == nb and got[0] == 1                                                  # E_1 = 3 <= 0.9 * 4
    got = rt.decide(En, Rate(budget=10), 2)                                              # a NaN gain never displaces an incumbent ...
    assert got.sum() == 10 and got[2] == 1 and got.tolist()[:2] == [3, 1]
    En[:, 0] = np.nan                                                                    # ... and as the first candidate it is never displaced
    assert rt.decide(En, Rate(budget=10), 2).tolist() == [3, 1, 1, 1, 1, 1, 1, 1]
    assert rt.decide(np.zeros((1, 7), np.float32), Rate(), 2).tolist() == [0, 0, 0, 0]   # no books: counts of 0


# ------------------------------------------------------------------------------------------------------- 3. Rate and frame
def test_rate_validation():
    assert Rate() == Rate(1, None, None) and Rate().resolve(8, 2) == (1, 0, 0.0, 0)
    assert Rate(2, tol2=0.84).resolve(8, 2) == (2, 1, float(np.float32(0.84)), 0)
    assert Rate(budget=20).resolve(8, 2) == (1, 2, 0.0, 20)
    for kw in (dict(tol2=0.5, budget=20), dict(min_books=0), dict(min_books=1.5), dict(tol2=0.0), dict(tol2=-1.0),
               dict(tol2=float("nan")), dict(tol2=float("inf")), dict(budget=2.5), dict(min_books=True)):
        with pytest.raises(ValueError):
            Rate(**kw)
    for rate, nb, ptok in ((Rate(min_books=9), 8, 2), (Rate(budget=7), 8, 2), (Rate(budget=65), 8, 2), (Rate(budget=8), 8, 1),
                           (Rate(min_books=3, budget=23), 8, 2), (Rate(), 8, 3), (Rate(), 8, 32), (Rate(), 8, 0)):
        with pytest.raises(ValueError):
            rate.resolve(nb, ptok)
    assert not hasattr(packets, "torch")                               # the host-side module stays numpy only


@pytest.mark.parametrize("K,nb,T,ptok", [(512, 8, 75, 2), (128, 10, 37, 4), (300, 3, 17, 16), (512, 8, 16, 1)])
def test_frame_with_one_count_per_packet_equals_thin(K, nb, T, ptok):
    info = StreamInfo(K, nb, T, ptok)
    r = np.random.default_rng(T)
    idx = r.integers(0, K, size=(nb, T))
    bodies = packets.pack_bodies(idx, info)
    whole = packets.frame(bodies, info)
    counts = r.integers(1, nb + 1, size=info.P)
    got = packets.frame(bodies, info, nb_sent=counts, seq_base=0)
    assert got == [packets.thin(whole[p], int(counts[p]), info) for p in range(info.P)]
    assert packets.frame(bodies, info, nb_sent=list(counts)) == got and packets.frame(bodies, info, nb_sent=nb) == whole
    g_bodies, g_recv = packets.gather(got, info)
    assert np.array_equal(g_recv, counts)
    back, nbv = packets.unpack_bodies(g_bodies, g_recv, info)
    assert np.array_equal(nbv, rt.expand(counts, T, ptok))
    assert np.array_equal(back, np.where(np.arange(nb)[:, None] < nbv[None, :], idx, 0))
    for bad in (counts[:-1], np.append(counts, 1), np.where(np.arange(info.P) == 0, 0, counts), np.where(np.arange(info.P) == 0, nb + 1, counts)):
        with pytest.raises(ValueError):
            packets.frame(bodies, info, nb_sent=bad)
    # the realised rate
    assert packets.sent_bits(counts, info) == 8 * sum(len(p) for p in got)
    assert packets.sent_bits(counts, info, headers=False) == 8 * sum(len(p) - packets.HEADER_BYTES for p in got)
    assert packets.sent_bits(nb, info) == 8 * sum(len(p) for p in whole)
    assert packets.sent_kbps(counts, info) == pytest.approx(packets.sent_bits(counts, info) * 75.0 / (1000.0 * T))


def test_sent_kbps_of_the_full_stream():
    info = StreamInfo(512, 8, 75, 2)                                   # 8 books x 9 bits x 75 tokens a second = 5.4 kbit/s of indices
    assert packets.sent_bits(8, info, headers=False) == 8 * (37 * 18 + 9)
    assert packets.sent_kbps(8, info, headers=False) == pytest.approx(5.4)
    assert packets.sent_kbps(8, info) == pytest.approx(5.4 + 38 * 72 / 1000.0)


# ---------------------------------------------------------------------------------------------------- 4. the design claim
@pytest.fixture(scope="module")
def model_sd():
    return {k: v.numpy() for k, v in synth.proposed_head_state(17, rvq_books=3, rvq_embed=128).items()}


@pytest.mark.parametrize("B,Tlat", [(2, 37), (1, 16), (1, 11)])
def test_closed_loop_z_run_equals_the_receivers(B, Tlat, orc, model_sd):
    r = np.random.default_rng(Tlat)
    qa = (0.5 * r.standard_normal((B, 1024, Tlat))).astype(np.float32)               # the audio latent both ends have (from the codes)
    zt = (0.5 * r.standard_normal((B, 1024, Tlat))).astype(np.float32)
    open_z, open_idx = __import__("sender_oracle").chunked_ar(orc, model_sd, qa, zt)
    seen = set()
    for rate in (Rate(), Rate(tol2=0.9), Rate(min_books=2, tol2=0.5), Rate(budget=14)):
        z_run, idx, nb_valid, nb_sent, _ = rt.closed_loop_ar(orc, model_sd, qa, zt, rate)
        assert idx.shape == (3, B, Tlat) and nb_valid.shape == (B, Tlat) and nb_sent.shape == (B, -(-Tlat // 2))
        assert np.array_equal(nb_valid, rt.expand(nb_sent, Tlat, 2))
        assert np.array_equal(z_run, lo.lossy_loop(orc, model_sd, qa, idx, nb_valid))
        assert np.array_equal(z_run, lo.lossy_two_pass(orc, model_sd, qa, idx, nb_valid))
        seen |= set(nb_sent.reshape(-1).tolist())
        if rate == Rate():                     # full rate, closed: the receiver's bits; the open loop is only round-off away
            assert np.all(nb_sent == 3) and np.array_equal(idx[:, :, :16], open_idx[:, :, :16])
            assert np.array_equal(z_run, ro.receiver_loop(orc, model_sd, qa, idx))
            assert not np.array_equal(z_run, open_z) and np.abs(z_run - open_z).max() < 1e-3 * np.abs(open_z).max()
    assert seen == {1, 2, 3}
    # the open loop thinned behind the sender's back does NOT reproduce at the receiver
    thin = np.full((B, Tlat), 1, np.uint8)
    assert not np.array_equal(open_z, lo.lossy_loop(orc, model_sd, qa, open_idx, thin))


# --------------------------------------------------------------------------------------------------------- 5. refusals, ABI
@pytest.fixture(scope="module")
def cpu_net():
    from multimodal_vqvae_compression_audio_tactile_amd import build_proposed
    return build_proposed(None, rvq_books=2, rvq_embed=128, device="cpu")


def test_rate_refusals_come_before_any_launch(cpu_net):
    """On a CPU-resident model nothing can have been launched: the checks come first."""
    from multimodal_vqvae_compression_audio_tactile_amd import ops
    net = cpu_net
    x = torch.zeros(1, 1, 5120)
    zt = torch.zeros(1, 1024, 16)
    calls = (lambda **kw: net.encode_latents_with_indices(x, x, **kw), lambda **kw: net.compress_packets(x, x, **kw),
             lambda **kw: net._ar_latents(zt, zt, **kw))
    for call in calls:
        with pytest.raises(ValueError, match="min_books"):
            call(rate=Rate(min_books=3))
        with pytest.raises(ValueError, match="budget"):
            call(rate=Rate(budget=17))
        with pytest.raises(ValueError, match="does not divide"):
            call(rate=Rate(), packet_tok=3)
        with pytest.raises(ValueError, match="packets.Rate"):
            call(rate=(1, None, None))
        with ops.arith("f16x3"):
            with pytest.raises(ValueError, match="arithmetic"):
                call(rate=Rate())
    with pytest.raises(ValueError, match="min_books"):
        net.encode_latents_with_indices(x, x, books_use=1, rate=Rate(min_books=2))
    with pytest.raises(ValueError, match="min_books"):
        net.stream_sender(rate=Rate(min_books=3))
    with pytest.raises(ValueError, match="budget"):
        net.stream_sender(packet_tok=4, rate=Rate(budget=9))
    with pytest.raises(ValueError, match="packets.Rate"):
        net.stream_sender(rate=(1, None, None))
    with ops.arith("f16x3"):
        with pytest.raises(ValueError, match="arithmetic"):
            net.stream_sender(rate=Rate())
    assert net.stream_sender(rate=Rate(budget=9)).rate == Rate(budget=9)


def test_rate_entry_points_are_exported_and_check_their_arguments():
    from multimodal_vqvae_compression_audio_tactile_amd import ProposedEval, StreamSender, _lib, ops
    import inspect
    lib = _lib.lib()
    for n in ("mvq_rvq_rate_f32", "mvq_ar_latents_staged_rate_f32"):
        assert n in _lib.EXPORTS and hasattr(lib, n), n
    assert callable(getattr(ops, "rvq_rate", None)) and callable(packets.sent_bits) and callable(packets.sent_kbps)
    for fn in (ProposedEval.encode_latents_with_indices, ProposedEval.compress_packets, ProposedEval.stream_sender,
               ProposedEval._ar_latents, StreamSender.__init__):
        assert "rate" in inspect.signature(fn).parameters, fn
    assert "rate" not in inspect.signature(ProposedEval.stream_sender_pool).parameters   # the pools are out of scope

    def rate(batch=1, dim=96, t=16, nb=8, k=512, ptok=2, gtok=16, mb=1, mode=0, tol2=0.0, budget=0):
        return lib.mvq_rvq_rate_f32(None, 0, 0, None, 0, 0, None, None, 0, 0, None, 0, None, 0, None, batch, dim, t, nb, k, ptok, gtok, mb,
                                    mode, tol2, budget, None)
    assert rate() == -1 and b"null" in lib.mvq_last_error()                              # a good shape gets as far as the tensors
    assert rate(batch=0) == 0 and rate(t=0) == 0
    for kw in (dict(batch=-1), dict(t=-1), dict(dim=0), dict(nb=-1), dict(k=0), dict(ptok=0), dict(ptok=3), dict(mb=0), dict(mb=9),
               dict(mode=3), dict(mode=1, tol2=0.0), dict(mode=1, tol2=float("nan")), dict(mode=1, tol2=float("inf")),
               dict(mode=2, budget=7), dict(mode=2, budget=65), dict(mode=2, budget=23, mb=3)):
        assert rate(**kw) == -1, kw
    assert rate(ptok=3) == -1 and b"divide" in lib.mvq_last_error()
    for kw in (dict(dim=98), dict(dim=132), dict(nb=33), dict(gtok=32)):
        assert rate(**kw) == -2, kw

    def staged(ptok=2, mb=1, mode=0, tol2=0.0, budget=0, **fields):
        a = _lib.ArArgs()
        a.batch, a.t_lat, a.t_audio, a.books_use, a.rvq_k = 1, 16, 16, 8, 512
        a.c_lat, a.c_ff, a.code_dim, a.heads, a.chunk = 1024, 2048, 96, 8, 16
        for n, v in fields.items():
            setattr(a, n, v)
        return lib.mvq_ar_latents_staged_rate_f32(ctypes.byref(a), ptok, mb, mode, tol2, budget, None, None, None, None, None, 0, None)
    assert staged() == -1 and b"null" in lib.mvq_last_error()
    assert staged(ptok=3) == -1 and b"divide" in lib.mvq_last_error()
    assert staged(mb=9) == -1 and b"min_books" in lib.mvq_last_error()
    assert staged(mode=2, budget=7) == -1 and b"budget" in lib.mvq_last_error()
    assert staged(mode=1, tol2=-1.0) == -1 and b"tol2" in lib.mvq_last_error()
    assert staged(batch=-1) == -1 and staged(t_lat=-1) == -1 and b"bad shape" in lib.mvq_last_error()
    assert lib.mvq_ar_latents_staged_rate_f32(None, 2, 1, 0, 0.0, 0, None, None, None, None, None, 0, None) == -1
