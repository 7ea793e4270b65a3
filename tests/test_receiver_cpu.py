"""CPU: the receiver's byte format (bitstream.py) and its arithmetic, restated from oracle pieces (tests/receiver_oracle.py).

  * pack / unpack round trips, the payload length is the reference's rate (kbps = tps * books * log2 K), corrupt input is rejected;
  * the receiver restatement against the transmitter (oracle.proposed_encode_latents): the worst |dz_run| measured here sets the
    GPU test's tolerance (tests/test_gpu_receiver.py, RX_VS_TX_REL);
  * the two-pass order equals the per-chunk loop bit for bit."""
from pathlib import Path

import numpy as np
import pytest
import torch

import golden_inputs as gi
import receiver_oracle as ro
from multimodal_vqvae_compression_audio_tactile_amd import bitstream, synth

from receiver_oracle import G4_PSNR_MEASURED, G4_Y_MEASURED, G4_Z_MEASURED, RX_VS_TX_MEASURED, RX_VS_TX_REL

G = Path(__file__).resolve().parent / "golden"


def _np(sd):
    return {k: v.numpy() for k, v in sd.items()}


@pytest.mark.parametrize("K", [128, 256, 512, 1000, 1024])
@pytest.mark.parametrize("nb", [1, 3, 8, 32])
@pytest.mark.parametrize("T", [0, 1, 35, 75, 2250])
def test_bitstream_round_trip(K, nb, T):
    r = np.random.default_rng(K * 7919 + nb * 31 + T)
    idx = r.integers(0, K, size=(nb, T))
    idx[:, :1] = K - 1                                               # the largest index survives
    blob = bitstream.pack_indices(idx, K)
    back, k = bitstream.unpack_indices(blob)
    assert k == K and back.dtype == np.int64 and back.shape == (nb, T)
    assert np.array_equal(back, idx)


@pytest.mark.parametrize("K,nb,T", [(512, 8, 75), (128, 10, 75), (1000, 3, 35), (1024, 32, 75), (512, 8, 0)])
def test_payload_length_is_the_reference_rate(K, nb, T):
    blob = bitstream.pack_indices(np.zeros((nb, T), np.int64), K)
    bits = T * nb * int(np.ceil(np.log2(K)))
    pad = (-bits) % 8
    assert 8 * len(blob) - 8 * bitstream.HEADER_BYTES - pad == bits
    if (K, nb, T) == (512, 8, 75):
        assert bits == 5400 and len(blob) - bitstream.HEADER_BYTES == 675      # 5.4 kbps at 75 tokens per second


def test_bit_layout_is_token_major_lsb_first():
    idx = np.array([[1, 2], [3, 0]])                                # nb = 2, T = 2, K = 4: 2 bits per index
    body = bitstream.pack_indices(idx, 4)[bitstream.HEADER_BYTES:]
    # token 0: book0 = 1 (bits 1,0), book1 = 3 (1,1); token 1: book0 = 2 (0,1), book1 = 0 (0,0)  -> 0b00_10_11_01
    assert body == bytes([0b00101101])


def test_corrupt_input_is_rejected():
    idx = np.arange(24).reshape(3, 8) % 128
    blob = bitstream.pack_indices(idx, 128)
    with pytest.raises(ValueError, match="truncated"):
        bitstream.unpack_indices(blob[:-1])
    with pytest.raises(ValueError):
        bitstream.unpack_indices(blob[:5])
    with pytest.raises(ValueError, match="magic"):
        bitstream.unpack_indices(b"XXXX" + blob[4:])
    with pytest.raises(ValueError, match="version"):
        bitstream.unpack_indices(blob[:4] + bytes([9]) + blob[5:])
    with pytest.raises(ValueError):
        bitstream.unpack_indices(blob + b"\0")
    # K = 1000 takes 10 bits: an all-ones index (1023) is representable but >= K
    bad = bytearray(bitstream.pack_indices(np.zeros((1, 4), np.int64), 1000))
    bad[bitstream.HEADER_BYTES] = 0xFF
    bad[bitstream.HEADER_BYTES + 1] |= 0x03
    with pytest.raises(ValueError, match=">= K"):
        bitstream.unpack_indices(bytes(bad))
    with pytest.raises(ValueError):
        bitstream.pack_indices(np.array([[0, 128]]), 128)
    with pytest.raises(ValueError):
        bitstream.pack_indices(np.array([[-1]]), 128)


def _rand_inputs(seed, B, Ta, Tlat, nb, K):
    r = np.random.default_rng(seed)
    qa = (0.5 * r.standard_normal((B, 1024, Ta))).astype(np.float32)
    idx = r.integers(0, K, size=(nb, B, Tlat))
    return qa, idx


@pytest.mark.parametrize("B,Ta,Tlat,use", [(2, 35, 35, None), (1, 20, 35, None), (1, 0, 35, None), (2, 75, 75, 2),
                                           (1, 16, 16, None), (1, 40, 33, None)])
def test_two_pass_equals_chunk_loop(B, Ta, Tlat, use, orc):
    """Only column 0 of a chunk s > 0 depends on the loop, so two dependent passes give the loop's bits exactly."""
    sd = _np(synth.proposed_head_state(17, rvq_books=3, rvq_embed=128))
    qa, idx = _rand_inputs(Ta * 100 + Tlat, B, Ta, Tlat, 3, 128)
    want = ro.receiver_loop(orc, sd, qa, idx, use)
    got = ro.receiver_two_pass(orc, sd, qa, idx, use)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("name", list(gi.PE_CASES))
def test_restatement_against_transmitter(name, orc):
    """The receiver (from the audio codes and the RVQ indices the transmitter produced) rebuilds the transmitter's z_run to
    round-off: the quantisers' straight-through sums are the only difference.  Also: qa from the codes matches the transmitter's
    qa to round-off."""
    books, K, use, B, seed = gi.PE_CASES[name]
    sd = _np(gi.model_state(seed, books, K))
    a, t = gi.pe_inputs(B, seed)
    z_tx, aux = orc.proposed_encode_latents(sd, a.numpy(), t.numpy(), use, return_aux=True)
    codes = orc.dac_quantizer(sd, aux["za"], prefix="A_QUANT.")[1]
    qa_rx, z_p = ro.from_codes(orc, sd, codes)
    assert z_p.shape == (B, 32 * 8, codes.shape[-1])
    assert np.abs(qa_rx - aux["qa"]).max() <= 1e-5 * np.abs(aux["qa"]).max()
    z_rx = ro.receiver_loop(orc, sd, qa_rx, aux["idx"], use)
    rel = np.abs(z_rx - z_tx).max() / np.abs(z_tx).max()
    print(f"{name}: receiver vs transmitter max |dz_run| / max|z_run| = {rel:.3g}")
    assert rel <= RX_VS_TX_MEASURED
    # qa passed directly (the transmitter's own) stays within the same bound
    z_rx2 = ro.receiver_loop(orc, sd, aux["qa"], aux["idx"], use)
    assert np.abs(z_rx2 - z_tx).max() / np.abs(z_tx).max() <= RX_VS_TX_MEASURED


@pytest.mark.parametrize("name", list(gi.PE_CASES))
def test_g4_codes_through_the_restatement(name, orc):
    """The reference's own transmitted codes (fixture G4) through the receiver restatement and T_DEC: z_run, the waveform and
    PSNR against G4's.  These measurements set the bounds of tests/test_gpu_receiver.py::test_g4_fixture_codes_to_waveform."""
    books, K, use, B, seed = gi.PE_CASES[name]
    g = np.load(G / "g4_proposed_eval.npz")
    sd = _np(gi.model_state(seed, books, K))
    _, t = gi.pe_inputs(B, seed)
    qa, _ = ro.from_codes(orc, sd, g[f"{name}.codes"].astype(np.int64))
    z = ro.receiver_loop(orc, sd, qa, g[f"{name}.idx"].astype(np.int64), use)
    want = g[f"{name}.z_run"]
    dz = np.abs(z - want).max() / np.abs(want).max()
    y = orc.dac_decoder(sd, z, prefix="T_DEC.")
    dy = np.abs(y - g[f"{name}.y"]).max()
    dp = np.abs(orc.psnr_batch(t.numpy()[..., :y.shape[-1]], y) - g[f"{name}.psnr"]).max()
    print(f"{name}: z_run rel {dz:.3g}, |dy| {dy:.3g}, PSNR {dp:.3g} dB")
    assert dz <= G4_Z_MEASURED and dy <= G4_Y_MEASURED and dp <= G4_PSNR_MEASURED


def test_decode_rejects_mismatched_batches_before_any_launch():
    """decode / decode_latents size every buffer from idx's batch: audio codes or qa of another batch are refused up front
    (on a CPU-resident model, so nothing could have been launched)."""
    from multimodal_vqvae_compression_audio_tactile_amd import MvqError, build_proposed
    net = build_proposed(None, rvq_books=2, rvq_embed=128, device="cpu")
    idx = torch.zeros(2, 2, 20, dtype=torch.int64)
    with pytest.raises(MvqError, match="batch"):
        net.decode(torch.zeros(1, 32, 20, dtype=torch.int64), idx)
    with pytest.raises(MvqError, match="batch"):
        net.decode_latents(torch.zeros(3, 32, 20, dtype=torch.int64), idx)
    with pytest.raises(MvqError, match="does not match"):
        net.decode_latents(idx=idx, qa=torch.zeros(1, 1024, 20))
    with pytest.raises(MvqError):
        net.decode_latents(torch.zeros(2, 20, dtype=torch.int64), idx)


def test_tactile_only_restatement(orc):
    """Tactile-only: z_run = proj_up(qD), the transmitter's tactile-only chain without the search."""
    books, K, use, B, seed = gi.PE_CASES["b3_k128_use2"]
    sd = _np(gi.model_state(seed, books, K))
    _, t = gi.pe_inputs(B, seed)
    z_tx, aux = orc.proposed_encode_latents(sd, None, t.numpy(), use, return_aux=True, tactile_only=True)
    z_rx = ro.receiver_loop(orc, sd, None, aux["idx"], use, tactile_only=True)
    assert np.abs(z_rx - z_tx).max() <= RX_VS_TX_REL * np.abs(z_tx).max()


def test_receiver_entry_points_exist():
    """The public surface the issue asks for (no GPU needed to look it up)."""
    from multimodal_vqvae_compression_audio_tactile_amd import ProposedEval, ResidualVectorQuantize, ResidualVQEMA, ops
    for obj, names in ((ProposedEval, ("decode", "decode_latents", "decode_latents_tactile_only", "decode_tactile_only",
                                       "compress", "decompress")),
                       (ResidualVectorQuantize, ("from_codes",)), (ResidualVQEMA, ("from_indices",)),
                       (ops, ("rvq_dequant", "dac_rvq_from_codes"))):
        for n in names:
            assert callable(getattr(obj, n, None)), n


def test_receiver_torch_ops_fakes():
    import multimodal_vqvae_compression_audio_tactile_amd.torch_ops as T
    o = torch.ops.mi355x_vqvae
    assert "rvq_dequant" in T.REGISTERED and "dac_rvq_from_codes" in T.REGISTERED
    m = lambda *s, dtype=torch.float32: torch.empty(*s, device="meta", dtype=dtype)
    assert o.rvq_dequant(m(3, 6, 75, dtype=torch.int64), m(8, 512, 96), 3).shape == (6, 96, 75)
    zq, zp = o.dac_rvq_from_codes(m(2, 32, 75, dtype=torch.int64), m(32, 1024, 8), m(32, 1024, 8), m(32, 1024))
    assert zq.shape == (2, 1024, 75) and zp.shape == (2, 256, 75)
