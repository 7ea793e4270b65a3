"""-m gpu: the receiver (ProposedEval.decode_latents / decode, ResidualVectorQuantize.from_codes, ResidualVQEMA.from_indices and
their kernels mvq_rvq_dequant_f32 / mvq_dac_rvq_from_codes_f32) against the CPU restatement of tests/receiver_oracle.py -- bit for
bit -- and against the G4 fixture of the reference's own classes to the bounds measured on the CPU (tests/receiver_oracle.py)."""
from pathlib import Path

import numpy as np
import pytest
import torch

import golden_inputs as gi
import receiver_oracle as ro
from receiver_oracle import G4_PSNR_DB, G4_Y_ATOL, G4_Z_REL, RX_VS_TX_REL

pytestmark = pytest.mark.gpu
G = Path(__file__).resolve().parent / "golden"

_NETS = {}


def _np(sd):
    return {k: v.numpy() for k, v in sd.items()}


def _net(books, K, seed, dev):
    key = (books, K, seed)
    if key not in _NETS:
        from multimodal_vqvae_compression_audio_tactile_amd import build_proposed
        sd = gi.model_state(seed, books, K)
        _NETS[key] = (build_proposed(sd, rvq_books=books, rvq_embed=K, device=dev), _np(sd))
    return _NETS[key]


@pytest.mark.parametrize("K,nb,use,B,T", [(128, 10, 10, 1, 75), (512, 3, 3, 6, 75), (1024, 10, 1, 256, 75), (512, 10, 3, 6, 35),
                                          (128, 3, 1, 256, 16), (1024, 3, 3, 1, 1), (512, 3, 3, 6, 0)])
def test_rvq_dequant_kernel_bit_exact(K, nb, use, B, T, dev):
    from multimodal_vqvae_compression_audio_tactile_amd import ops
    z, books = gi.rvq_inputs(K, nb, 1, 1, 500 + K + B)
    r = np.random.default_rng(K + nb + B + T)
    idx = r.integers(0, K, size=(nb, B, T))
    bk = torch.from_numpy(np.stack(books)).to(dev)
    got = ops.rvq_dequant(torch.from_numpy(idx).to(dev), bk, use)
    want = ro.dequant(books, idx, use)
    assert got.shape == (B, 96, T)
    assert np.array_equal(got.cpu().numpy(), want)
    # the token-folded layout the receiver's GEMMs read: [1, 96, B*T]
    fold = torch.empty(1, 96, B * T, device=dev)
    ops.rvq_dequant(torch.from_numpy(idx).to(dev), bk, use, out=fold, out_strides=(T, B * T))
    assert np.array_equal(fold.cpu().numpy().reshape(96, B, T).transpose(1, 0, 2), want)


def test_rvq_dequant_clamps_corrupt_indices(dev):
    from multimodal_vqvae_compression_audio_tactile_amd import ops
    _, books = gi.rvq_inputs(128, 2, 1, 1, 77)
    idx = np.array([[[0, 5000, -3, 127]], [[-1, 2, 128, 9]]], np.int64)
    got = ops.rvq_dequant(torch.from_numpy(idx).to(dev), torch.from_numpy(np.stack(books)).to(dev))
    assert np.array_equal(got.cpu().numpy(), ro.dequant(books, np.clip(idx, 0, 127)))


def test_rvq_dequant_zero_books_and_default_strides(dev):
    """nb_use = 0 writes zeros; out strides (0, 0) at the C ABI mean the plain [B, D, T] layout."""
    from multimodal_vqvae_compression_audio_tactile_amd import _lib, ops
    _, books = gi.rvq_inputs(128, 3, 1, 1, 78)
    bk = torch.from_numpy(np.stack(books)).to(dev)
    idx = torch.from_numpy(np.random.default_rng(3).integers(0, 128, size=(3, 6, 20))).to(dev)
    out = torch.full((6, 96, 20), float("nan"), device=dev)
    ops.rvq_dequant(idx, bk, 0, out=out, out_strides=(96 * 20, 20))
    assert torch.equal(out, torch.zeros_like(out))
    out.fill_(float("nan"))
    rc = _lib.lib().mvq_rvq_dequant_f32(idx.data_ptr(), bk.data_ptr(), out.data_ptr(), 6, 96, 20, 3, 128, 0, 0,
                                        torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), ro.dequant(books, idx.cpu().numpy()))


def test_receiver_ops_refuse_what_would_reach_out_of_bounds(dev):
    """Host-side checks, before any launch: an out buffer too small for its strides, mis-shaped out_proj weights, batches that
    do not match."""
    from multimodal_vqvae_compression_audio_tactile_amd import MvqError, ops
    _, books = gi.rvq_inputs(128, 2, 1, 1, 79)
    bk = torch.from_numpy(np.stack(books)).to(dev)
    idx = torch.zeros(2, 2, 20, dtype=torch.int64, device=dev)
    with pytest.raises(MvqError, match="reaches past"):
        ops.rvq_dequant(idx, bk, out=torch.empty(1, 96, 20, device=dev), out_strides=(96 * 20, 20))
    with pytest.raises(MvqError):
        ops.rvq_dequant(idx, bk, out=torch.empty(2, 96, 20, device=dev, dtype=torch.float64), out_strides=(96 * 20, 20))
    codes = torch.zeros(1, 8, 10, dtype=torch.int64, device=dev)
    cb = torch.zeros(8, 1024, 8, device=dev)
    with pytest.raises(MvqError):
        ops.dac_rvq_from_codes(codes, cb, torch.zeros(4, 1024, 8, device=dev), torch.zeros(8, 1024, device=dev))
    with pytest.raises(MvqError):
        ops.dac_rvq_from_codes(codes, cb, torch.zeros(8, 1024, 8, device=dev), torch.zeros(8, 512, device=dev))
    net, _ = _net(8, 512, 7, dev)
    idx = torch.zeros(8, 2, 75, dtype=torch.int64, device=dev)
    with pytest.raises(MvqError, match="batch"):
        net.decode(torch.zeros(1, 32, 75, dtype=torch.int64, device=dev), idx)
    # a float64 qa is taken as fp32 values, not as raw bytes
    qa = torch.from_numpy(np.random.default_rng(4).standard_normal((2, 1024, 75)).astype(np.float32)).to(dev)
    assert torch.equal(net.decode_latents(idx=idx, qa=qa.double()), net.decode_latents(idx=idx, qa=qa))


@pytest.mark.parametrize("nq,B,T", [(1, 1, 75), (8, 6, 75), (32, 256, 75), (32, 1, 35), (8, 6, 0), (32, 6, 1)])
def test_from_codes_kernel_bit_exact(nq, B, T, dev, orc):
    net, sd = _net(8, 512, 7, dev)
    r = np.random.default_rng(nq * 1000 + B + T)
    codes = r.integers(0, 1024, size=(B, nq, T))
    z_q, z_p, c_out = net.A_QUANT.from_codes(torch.from_numpy(codes).to(dev))
    assert z_q.shape == (B, 1024, T) and z_p.shape == (B, nq * 8, T) and c_out.shape == codes.shape
    if T == 0:
        return
    want_q, want_p = ro.from_codes(orc, sd, codes)
    assert np.array_equal(z_p.cpu().numpy(), want_p)
    assert np.array_equal(z_q.cpu().numpy(), want_q)


@pytest.mark.parametrize("K", [128, 1024])
def test_from_codes_other_codebook_sizes_and_clamp(K, dev, orc):
    """K is a kernel argument: a quantiser with another codebook size; out-of-range codes are clamped, never read past the book."""
    from multimodal_vqvae_compression_audio_tactile_amd import ops
    r = np.random.default_rng(K)
    cb = (r.standard_normal((8, K, 8)) * 0.3).astype(np.float32)
    ow = (r.standard_normal((8, 1024, 8)) * 0.2).astype(np.float32)
    ob = (r.standard_normal((8, 1024)) * 0.1).astype(np.float32)
    codes = r.integers(0, K, size=(6, 8, 20))
    codes[0, 0, 0], codes[1, 3, 5] = K + 7, -2
    t = lambda x: torch.from_numpy(x).to(dev)
    z_q, z_p = ops.dac_rvq_from_codes(t(codes), t(cb), t(ow), t(ob))
    cc = np.clip(codes, 0, K - 1)
    want_p = np.concatenate([cb[i][cc[:, i]].transpose(0, 2, 1) for i in range(8)], axis=1)
    want_q = None
    for i in range(8):
        zi = orc.conv1d(np.ascontiguousarray(cb[i][cc[:, i]].transpose(0, 2, 1)), ow[i][:, :, None], ob[i])
        want_q = np.zeros_like(zi) + zi if want_q is None else want_q + zi
    assert np.array_equal(z_p.cpu().numpy(), want_p)
    assert np.array_equal(z_q.cpu().numpy(), want_q)


@pytest.mark.parametrize("name", list(gi.PE_CASES))
def test_decode_latents_bit_exact_vs_chunk_loop(name, dev, orc):
    """From the transmitter's own outputs (codes [B,32,Ta] int64, idx [nb,B,Tlat] int64): bit-equal to the per-chunk
    receiver loop, and within round-off of the transmitter's z_run."""
    books, K, use, B, seed = gi.PE_CASES[name]
    net, sd = _net(books, K, seed, dev)
    a, t = gi.pe_inputs(B, seed)
    z_tx, codes, idx = net.encode_latents_with_indices(a.to(dev), t.to(dev), books_use=use)
    assert codes.dtype == torch.int64 and idx.dtype == torch.int64
    z_rx = net.decode_latents(codes, idx)
    qa, _ = ro.from_codes(orc, sd, codes.cpu().numpy())
    want = ro.receiver_loop(orc, sd, qa, idx.cpu().numpy())
    assert np.array_equal(z_rx.cpu().numpy(), want)
    assert (z_rx - z_tx).abs().max().item() <= RX_VS_TX_REL * z_tx.abs().max().item()
    # books_use on the receiver side limits the books it sums
    if use is None:
        z2 = net.decode_latents(codes, idx, books_use=2)
        assert np.array_equal(z2.cpu().numpy(), ro.receiver_loop(orc, sd, qa, idx.cpu().numpy(), 2))


def test_decode_latents_tactile_only(dev, orc):
    books, K, use, B, seed = gi.PE_CASES["b3_k128_use2"]
    net, sd = _net(books, K, seed, dev)
    _, t = gi.pe_inputs(B, seed)
    z_tx = net.encode_latents_tactile_only(t.to(dev), books_use=use)
    zt = net.T_ENC(t.to(dev))
    _, _, idx = net._ar_latents(None, zt, use, tactile_only=True, want_indices=True)
    z_rx = net.decode_latents_tactile_only(idx)
    assert np.array_equal(z_rx.cpu().numpy(), ro.receiver_loop(orc, sd, None, idx.cpu().numpy(), tactile_only=True))
    assert (z_rx - z_tx).abs().max().item() <= RX_VS_TX_REL * z_tx.abs().max().item()
    y = net.decode_tactile_only(idx)
    assert torch.equal(y, net.T_DEC(z_rx))


@pytest.mark.parametrize("Ta,Tlat", [(20, 35), (0, 35), (9, 16), (40, 33)])
def test_decode_latents_audio_shorter_than_tactile(Ta, Tlat, dev, orc):
    """Whole-file mode: chunks with ka < 16 and ka = 0 attend to what audio there is (Tk = 0: no context), as the transmitter."""
    net, sd = _net(3, 128, 9, dev)
    r = np.random.default_rng(Ta * 100 + Tlat)
    qa = (0.5 * r.standard_normal((2, 1024, Ta))).astype(np.float32)
    idx = r.integers(0, 128, size=(3, 2, Tlat))
    got = net.decode_latents(idx=torch.from_numpy(idx).to(dev), qa=torch.from_numpy(qa).to(dev))
    assert np.array_equal(got.cpu().numpy(), ro.receiver_loop(orc, sd, qa, idx))


def test_decode_latents_b256_planted_rows(dev, orc):
    """B = 256 one-second segments: three planted rows equal their B = 1 runs (and those equal the restatement)."""
    net, sd = _net(8, 512, 7, dev)
    r = np.random.default_rng(256)
    B, Tlat = 256, 75
    qa = torch.from_numpy((0.5 * r.standard_normal((B, 1024, Tlat))).astype(np.float32)).to(dev)
    idx = torch.from_numpy(r.integers(0, 512, size=(8, B, Tlat))).to(dev)
    z = net.decode_latents(idx=idx, qa=qa)
    for b in (0, 131, 255):
        one = net.decode_latents(idx=idx[:, b:b + 1], qa=qa[b:b + 1])
        assert torch.equal(z[b:b + 1], one), b
    want = ro.receiver_loop(orc, sd, qa[131:132].cpu().numpy(), idx[:, 131:132].cpu().numpy())
    assert np.array_equal(z[131:132].cpu().numpy(), want)


@pytest.mark.parametrize("name", list(gi.PE_CASES))
def test_g4_fixture_codes_to_waveform(name, dev):
    """The reference's own transmitted codes (G4) decoded by the receiver: z_run within the CPU-measured receiver-vs-transmitter
    bound of G4's z_run, the waveform within G4_Y_ATOL of G4's, PSNR within G4_PSNR_DB (10x what the CPU restatement shows,
    tests/receiver_oracle.py)."""
    from multimodal_vqvae_compression_audio_tactile_amd import psnr_batch
    books, K, use, B, seed = gi.PE_CASES[name]
    net, _ = _net(books, K, seed, dev)
    g = np.load(G / "g4_proposed_eval.npz")
    codes = torch.from_numpy(g[f"{name}.codes"].astype(np.int64)).to(dev)
    idx = torch.from_numpy(g[f"{name}.idx"].astype(np.int64)).to(dev)
    z = net.decode_latents(codes, idx).cpu().numpy()
    want = g[f"{name}.z_run"]
    assert np.abs(z - want).max() <= G4_Z_REL * np.abs(want).max()
    y = net.decode(codes, idx)
    np.testing.assert_allclose(y.cpu().numpy(), g[f"{name}.y"], rtol=0, atol=G4_Y_ATOL)
    _, t = gi.pe_inputs(B, seed)
    p = np.array(psnr_batch(t[..., :y.shape[-1]].to(dev), y))
    assert np.max(np.abs(p - g[f"{name}.psnr"])) <= G4_PSNR_DB


def test_compress_decompress_round_trip(dev):
    from multimodal_vqvae_compression_audio_tactile_amd import bitstream, synth
    net, _ = _net(8, 512, 7, dev)
    a, t = synth.audio_segments(2, seed=3), synth.tactile_segments(2, seed=3)          # two 1-s segments
    tac, aud = net.compress(a.to(dev), t.to(dev))
    assert len(tac) == len(aud) == 2
    assert all(len(p) == bitstream.HEADER_BYTES + 675 for p in tac)                      # 8 books x 9 bits x 75 tokens
    assert all(len(p) == bitstream.HEADER_BYTES + 32 * 10 * 75 // 8 for p in aud)
    y = net.decompress(tac, aud)
    _, codes, idx = net.encode_latents_with_indices(a.to(dev), t.to(dev))
    assert torch.equal(y, net.decode(codes, idx))
    with pytest.raises(ValueError):
        net.decompress([tac[0][:-3]], [aud[0]])


def test_decode_graph_capture_replays_bit_equal(dev):
    net, _ = _net(8, 512, 7, dev)
    r = np.random.default_rng(5)
    codes = torch.from_numpy(r.integers(0, 1024, size=(2, 32, 75))).to(dev)
    idx = torch.from_numpy(r.integers(0, 512, size=(8, 2, 75))).to(dev)
    want = net.decode(codes, idx)
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        net.decode(codes, idx)                                   # warm the caches outside the capture
        with torch.cuda.graph(g, stream=s):
            got = net.decode(codes, idx)
    torch.cuda.current_stream().wait_stream(s)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(got, want)
