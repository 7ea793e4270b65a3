"""CPU: the packet-loss-concealment surface without a device -- AllPredPLC's constructor and state-dict layout (fixture G16),
the new C-ABI entry points (declared, exported, refusing bad arguments before any launch) and the token-loss mask mirror
against the mask the reference drew (fixture G13)."""
import ctypes
import inspect
import json
import re
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
NEW = ("mvq_attention_seq_f32", "mvq_attention_seq_bwd_scratch_bytes", "mvq_attention_seq_bwd_f32", "mvq_plc_mask_fill_f32",
       "mvq_plc_mask_fill_bwd_f32")


def test_plc_state_dict_matches_the_reference_layout():
    import multimodal_vqvae_compression_audio_tactile_amd as mvq
    import plc_inputs as pi
    assert list(inspect.signature(mvq.AllPredPLC.__init__).parameters) == ["self", "A_ENC", "A_QUANT", "T_ENC", "T_DEC", "c_lat"]
    da, dt = mvq.DAC(), mvq.DAC()
    net = mvq.AllPredPLC(da.encoder, da.quantizer, dt.encoder, dt.decoder, c_lat=1024)
    want = json.loads((ROOT / "tests" / "golden" / "g16_plc_state_shapes.json").read_text())
    assert {k: list(v.shape) for k, v in net.state_dict().items()} == want
    assert isinstance(net.predict, mvq.CrossPredictor) and isinstance(net.tokennorm, mvq.TokenNorm)
    assert not any(p.requires_grad for m in (net.A_ENC, net.A_QUANT, net.T_ENC, net.T_DEC) for p in m.parameters())
    res = net.load_state_dict({"model": pi.plc_state()}["model"], strict=True)          # PLC1_eval.py: load ckpt["model"]
    assert not res.missing_keys and not res.unexpected_keys


def test_new_entry_points_are_declared_and_exported():
    from multimodal_vqvae_compression_audio_tactile_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mvq.h").read_text(), flags=re.S)
    so = ctypes.CDLL(str(_lib.SO_PATH))
    for n in NEW:
        assert re.search(rf"\b{n}\s*\(", txt), n
        assert hasattr(so, n) and n in _lib.EXPORTS, n
    assert _lib.lib().mvq_abi_version() == 3


def test_new_entry_points_refuse_bad_arguments_without_a_device():
    from multimodal_vqvae_compression_audio_tactile_amd import _lib
    lib = _lib.lib()
    fake = 4096                                                          # never dereferenced: every call below is refused first
    # oversize (8193 tokens) and null tensors
    assert lib.mvq_attention_seq_f32(fake, fake, fake, fake, 1, 8, 128, 8193, 75, 0, 0, 0, 0, None) == -1
    assert lib.mvq_attention_seq_f32(fake, fake, fake, fake, 1, 8, 128, 75, 8193, 0, 0, 0, 0, None) == -1
    assert lib.mvq_attention_seq_f32(None, None, None, None, 1, 8, 128, 75, 75, 0, 0, 0, 0, None) == -1
    assert lib.mvq_attention_seq_f32(fake, fake, fake, fake, 1, 8, 4096, 75, 75, 0, 0, 0, 0, None) == -1     # dh too wide for LDS
    assert lib.mvq_attention_seq_f32(None, None, None, None, 0, 8, 128, 75, 75, 0, 0, 0, 0, None) == 0       # empty batch
    assert lib.mvq_attention_seq_bwd_f32(fake, fake, fake, fake, fake, fake, fake, fake, 1, 8, 128, 513, 75, 0, 0, 0, 0, None) == -1
    assert lib.mvq_attention_seq_bwd_f32(fake, fake, fake, fake, fake, fake, fake, fake, 1, 8, 128, 75, 513, 0, 0, 0, 0, None) == -1
    assert lib.mvq_attention_seq_bwd_f32(None, None, None, None, None, None, None, None, 1, 8, 128, 75, 75, 0, 0, 0, 0, None) == -1
    assert lib.mvq_attention_seq_bwd_f32(fake, fake, fake, fake, fake, fake, fake, fake + 4, 1, 8, 128, 75, 75, 0, 0, 0, 0, None) == -1
    assert lib.mvq_attention_seq_bwd_scratch_bytes(6, 8, 75, 75) == 2 * 6 * 8 * 75 * 75 * 4
    assert lib.mvq_plc_mask_fill_f32(None, None, None, None, None, 2, 1024, 75, 0, 0, None) == -1
    assert lib.mvq_plc_mask_fill_f32(fake, None, fake, None, fake, 2, 1024, 75, 0, 0, None) == -1            # z_filled needs z_pred
    assert lib.mvq_plc_mask_fill_bwd_f32(None, None, None, 2, 1024, 75, 0, 0, None) == -1
    assert b"null" in lib.mvq_last_error()


def test_mask_mirror_draws_the_reference_mask_on_the_cpu_generator():
    """make_token_loss_mask issues the reference's single torch.rand(B, P): with the same seed on the CPU it returns the mask
    G13 stored from the reference (including the never-lost pad token of an odd T_lat)."""
    from multimodal_vqvae_compression_audio_tactile_amd import make_token_loss_mask
    import plc_inputs as pi
    G13 = np.load(ROOT / "tests" / "golden" / "g13_plc_forward.npz")
    for name, (B, Tw, seed) in pi.FWD_CASES.items():
        T_lat = Tw // 320
        torch.manual_seed(pi.MASK_SEED + seed)
        m = make_token_loss_mask(B, T_lat, 2, 0.5, "cpu")
        assert m.dtype == torch.bool and tuple(m.shape) == (B, T_lat)
        assert np.array_equal(m.numpy(), G13[f"{name}.mask"]), name
        assert not m[:, -1].any()                                        # 75 / 225 tokens: the last one is padding
    assert make_token_loss_mask(2, 0, 2, 0.5, "cpu").shape == (2, 0)
    assert make_token_loss_mask(1, 1, 2, 0.5, "cpu").shape == (1, 1)      # one packet, cropped to one token
