"""Packet-loss concealment (PLC) on libmvq_hip.so: the reference's ``AllPredPLC`` (PLC/PLC1.py:349-422, the same class in
PLC/PLC1_eval.py and PLC/PLC1_low_mid_high*.py), its token-loss mask and the masked / unmasked waveform metrics of
PLC/PLC1_eval.py:200-224,620-663.

The model is the compression model's frozen DAC encoders / decoder and the same ``CrossPredictor``, called ONCE over the
whole latent sequence instead of per 16-token AR chunk:

    zt_in = T_ENC(tc) * ~mask;  z_pred = predict(zt_in, A_QUANT(A_ENC(a))[0]);  y_hat = T_DEC(where(mask, z_pred, zt_in))

so its attention runs on the full-sequence kernels (ops.attention_seq, Tq = Tk = T_lat up to 8192) and the fill on
``mvq_plc_mask_fill_f32``.  With autograd enabled ``forward_step`` records the HIP graph of train.py (gradients reach
``predict.*`` through the decoder input-gradient, PlcFill and the predictor, with ctx dropout in train mode); under
``torch.no_grad()`` it is the inference path.  ``tokennorm`` exists in the reference but is unused by its forward pass: it
is kept (same state-dict keys) and stays unused.
"""
from __future__ import annotations

from typing import Callable, Optional

import torch
import torch.nn as nn

from . import ops, train
from .proposed import CrossPredictor, TokenNorm

PACKET_TOK = 2            # PLC/PLC1.py:68
PACKET_LOSS_PROB = 0.5    # ...:69
METRIC_EPS = 1e-12        # PLC/PLC1_eval.py:85


def make_token_loss_mask(batch_size: int, T_lat: int, packet_tok: int, p_loss: float, device) -> torch.Tensor:
    """Packet loss on latent tokens (PLC/PLC1.py:326-347): each packet of ``packet_tok`` tokens is lost with probability
    ``p_loss``.  One ``torch.rand(B, P)`` draw (P = max(1, T_lat // packet_tok)) on ``device``, so the same seed on the same
    device gives the reference's mask; tokens past P * packet_tok (odd T_lat) are never lost.  -> bool [B, T_lat]."""
    if packet_tok <= 0 or T_lat <= 0:
        return torch.zeros(batch_size, T_lat, dtype=torch.bool, device=device)
    n_packets = max(1, T_lat // packet_tok)
    lost = torch.rand(batch_size, n_packets, device=device) < p_loss
    tokens = lost.repeat_interleave(packet_tok, dim=1)
    n = tokens.shape[1]
    if n >= T_lat:
        return tokens[:, :T_lat].contiguous()
    tail = torch.zeros(batch_size, T_lat - n, dtype=torch.bool, device=device)
    return torch.cat([tokens, tail], dim=1)


class AllPredPLC(nn.Module):
    """PLC/PLC1.py:349-422: constructor ``(A_ENC, A_QUANT, T_ENC, T_DEC, c_lat)``, attributes ``predict`` / ``tokennorm``, the
    reference's state-dict keys.  ``forward_step(a, tc)`` draws the mask as the reference does; ``mask=`` ([B, T_lat] or
    [B, 1, T_lat], True = lost) fixes it, ``mask_fn(B, T_lat, device)`` supplies another policy (e.g. the category bursts of
    PLC/PLC1_low_mid_high.py, host logic whose mask is all that differs between the two models)."""

    def __init__(self, A_ENC, A_QUANT, T_ENC, T_DEC, c_lat):
        super().__init__()
        self.A_ENC, self.A_QUANT, self.T_ENC, self.T_DEC = A_ENC, A_QUANT, T_ENC, T_DEC
        for m in [self.A_ENC, self.A_QUANT, self.T_ENC, self.T_DEC]:
            for p in m.parameters():
                p.requires_grad_(False)
        self.predict = CrossPredictor(c=c_lat, heads=8, mlp_mul=2, dropout=0.1)
        self.tokennorm = TokenNorm(c_lat)

    def _mask(self, B, T_lat, device, mask, mask_fn):
        if mask is not None:
            m = mask.reshape(B, T_lat) if mask.dim() == 3 else mask
            if tuple(m.shape) != (B, T_lat):
                raise ValueError(f"AllPredPLC: mask of shape {tuple(mask.shape)} for B={B}, T_lat={T_lat}")
            return m.to(device=device, dtype=torch.bool)
        if mask_fn is not None:
            return mask_fn(B, T_lat, device).to(dtype=torch.bool)
        return make_token_loss_mask(B, T_lat, PACKET_TOK, PACKET_LOSS_PROB, device)

    def forward_step(self, a_1T, tc_1T, mask: Optional[torch.Tensor] = None,
                     mask_fn: Optional[Callable[[int, int, torch.device], torch.Tensor]] = None):
        """a_1T, tc_1T: [B,1,T_wav] -> {"y_hat", "tgt", "latent_mask" [B,1,T_lat] bool}."""
        Tw = tc_1T.shape[-1]
        with torch.no_grad():                                                   # frozen backbones: no graph
            qa, *_ = self.A_QUANT(self.A_ENC(a_1T))
            zt = self.T_ENC(tc_1T)
        B, C, T_lat = zt.shape
        m = self._mask(B, T_lat, zt.device, mask, mask_fn)
        zt_in, _ = ops.plc_mask_fill(zt, None, m)                               # zt * ~mask: what the receiver sees
        if torch.is_grad_enabled() and T_lat and any(p.requires_grad for p in self.predict.parameters()):
            z_pred = self.predict(zt_in, qa)                                    # run_train: full-sequence attention + bwd
            z_filled = train.PlcFill.apply(zt, z_pred, m, None)
            y_hat = self.T_DEC(z_filled)                                        # HIP input-gradient of the frozen decoder
        else:
            with torch.no_grad():
                z_pred = self.predict(zt_in, qa) if T_lat else zt_in      # refuses train-mode dropout without autograd
                _, z_filled = ops.plc_mask_fill(zt, z_pred, m, want_zt_in=False)
                y_hat = self.T_DEC(z_filled)
        T = min(y_hat.shape[-1], tc_1T.shape[-1], Tw)
        fz = lambda x: torch.nan_to_num(x, nan=0.0, posinf=0.0, neginf=0.0)    # finite_or_zero (PLC1.py:94-95)
        return {"y_hat": fz(y_hat[..., :T]), "tgt": fz(tc_1T[..., :T]), "latent_mask": m.unsqueeze(1)}


# ---------------------------------------------------------------------- masked / unmasked metrics (PLC/PLC1_eval.py:200-224)
def token_to_sample_mask(latent_mask: torch.Tensor, T_wave: int) -> torch.Tensor:
    """Token mask [T_lat] -> sample mask [T_wave]: sample n belongs to token floor(n / (T_wave / T_lat)) computed in float32,
    clamped to [0, T_lat-1] (PLC/PLC1_eval.py:652-656)."""
    lm = latent_mask.reshape(-1).bool()
    T_lat = lm.numel()
    if T_lat == 0 or T_wave == 0:
        return torch.zeros(T_wave, dtype=torch.bool, device=lm.device)
    spt = float(T_wave) / float(T_lat)
    idx = torch.arange(T_wave, dtype=torch.float32, device=lm.device)
    tok = torch.floor(idx / spt).long().clamp_(0, T_lat - 1)
    return lm[tok]


def _subset(ref_vec, est_vec, mask):
    m = mask.to(device=ref_vec.device, dtype=torch.bool)
    if not bool(m.any()):
        return None
    return ref_vec[m].to(torch.float32), est_vec.to(ref_vec.device)[m].to(torch.float32)


def mae_subset(ref_vec, est_vec, mask) -> float:
    """mean |ref - est| over the samples where mask is True; NaN on an empty subset."""
    s = _subset(ref_vec, est_vec, mask)
    return float("nan") if s is None else float((s[0] - s[1]).abs().mean())


def snr_subset_db(ref_vec, est_vec, mask, eps: float = METRIC_EPS) -> float:
    """10 log10(mean r^2 / (mean (r-e)^2 + eps)) over the subset; NaN on an empty subset."""
    s = _subset(ref_vec, est_vec, mask)
    if s is None:
        return float("nan")
    r, e = s
    return float(10.0 * torch.log10(torch.mean(r ** 2) / (torch.mean((r - e) ** 2) + eps)))


def psnr_subset_db(ref_vec, est_vec, mask, peak: float, eps: float = METRIC_EPS) -> float:
    """10 log10(peak^2 / (mean (r-e)^2 + eps)) over the subset with peak = max(peak, eps); NaN on an empty subset."""
    s = _subset(ref_vec, est_vec, mask)
    if s is None:
        return float("nan")
    r, e = s
    pk = max(float(peak), eps)
    return float(10.0 * torch.log10((pk * pk) / (torch.mean((r - e) ** 2) + eps)))


def masked_metrics(ref_vec, est_vec, latent_mask, peak: float) -> dict:
    """The six masked / unmasked figures PLC/PLC1_eval.py:646-663 reports for one aligned file."""
    T_wave = ref_vec.numel()
    if latent_mask.numel() == 0 or T_wave == 0:
        nan = float("nan")
        return {k: nan for k in ("mae_masked", "mae_unmasked", "snr_masked", "snr_unmasked", "psnr_masked", "psnr_unmasked")}
    sm = token_to_sample_mask(latent_mask.to(ref_vec.device), T_wave)
    r, e = ref_vec.reshape(-1), est_vec.reshape(-1)
    return {"mae_masked": mae_subset(r, e, sm), "mae_unmasked": mae_subset(r, e, ~sm),
            "snr_masked": snr_subset_db(r, e, sm), "snr_unmasked": snr_subset_db(r, e, ~sm),
            "psnr_masked": psnr_subset_db(r, e, sm, peak), "psnr_unmasked": psnr_subset_db(r, e, ~sm, peak)}

