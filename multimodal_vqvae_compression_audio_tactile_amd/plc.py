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

import math
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
                     mask_fn: Optional[Callable[[int, int, torch.device], torch.Tensor]] = None, *, na_valid=None,
                     audio_conceal="zero"):
        """a_1T, tc_1T: [B,1,T_wav] -> {"y_hat", "tgt", "latent_mask" [B,1,T_lat] bool}.
        ``na_valid`` (uint8 [B, Ta] on the device: the audio stages of each token that arrive) / ``audio_conceal`` ("zero",
        "mask", "hold"): the audio side as the receiver reconstructs it under loss (decode_latents) -- qa from the codes with the
        stages that arrived, then "hold" fills lost tokens and "mask" takes them out of the predictor's keys (masked
        full-sequence attention and its backward, T_lat <= 512 under autograd).  Defaults: the reference's step."""
        if na_valid is not None or audio_conceal != "zero":
            return self._forward_step_link(a_1T, tc_1T, mask, mask_fn, na_valid, audio_conceal)
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


    def _forward_step_link(self, a_1T, tc_1T, mask, mask_fn, na_valid, audio_conceal):
        from .proposed import link_step_refusals
        link_step_refusals("AllPredPLC.forward_step", self, a_1T, tc_1T, None, na_valid, audio_conceal, None)
        Tw = tc_1T.shape[-1]
        with torch.no_grad():                                                   # frozen backbones: no graph
            _, codes, *_ = self.A_QUANT(self.A_ENC(a_1T))
            zt = self.T_ENC(tc_1T)
            B, C, T_lat = zt.shape
            if tuple(na_valid.shape) != (B, codes.shape[2]):
                raise ValueError(f"AllPredPLC: na_valid {tuple(na_valid.shape)} does not match the codes' [B={B}, Ta={codes.shape[2]}]")
            na_valid = na_valid.contiguous()
            qa = ops._dev(self.A_QUANT.from_codes(codes, nq_valid=na_valid)[0], "qa")
            if audio_conceal == "hold":
                ops.hold_fill_(qa, na_valid)
        key_mask = na_valid if audio_conceal == "mask" else None
        m = self._mask(B, T_lat, zt.device, mask, mask_fn)
        zt_in, _ = ops.plc_mask_fill(zt, None, m)
        y_hat = self._fill_decode(zt, zt_in, qa, m, key_mask)
        T = min(y_hat.shape[-1], tc_1T.shape[-1], Tw)
        fz = lambda x: torch.nan_to_num(x, nan=0.0, posinf=0.0, neginf=0.0)
        return {"y_hat": fz(y_hat[..., :T]), "tgt": fz(tc_1T[..., :T]), "latent_mask": m.unsqueeze(1), "codes": codes,
                "na_valid": na_valid}

    def _fill_decode(self, zt, zt_in, qa, m, key_mask):
        """z_pred = predict(zt_in, qa) under ``key_mask``, the fill and the decoder: recorded under autograd (run_train, called
        directly: CrossPredictor.forward keeps key_mask for inference), the inference kernels without."""
        B, C, T_lat = zt.shape
        if torch.is_grad_enabled() and T_lat and any(p.requires_grad for p in self.predict.parameters()):
            fold = lambda x: x.permute(1, 0, 2).reshape(1, C, -1).contiguous()
            z_pred = self.predict.run_train(fold(zt_in), fold(qa), B, key_mask=key_mask)
            z_pred = z_pred.reshape(C, B, T_lat).permute(1, 0, 2).contiguous()
            return self.T_DEC(train.PlcFill.apply(zt, z_pred, m, None))
        with torch.no_grad():
            z_pred = self.predict(zt_in, qa, key_mask=key_mask) if T_lat else zt_in
            return self.T_DEC(ops.plc_mask_fill(zt, z_pred, m, want_zt_in=False)[1])


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



# ------------------------------------------ mel ST-SIM and the pass-1 file evaluation (PLC/PLC1_eval.py:270-333,585-663)
TARGET_SR = 24000         # PLC/PLC1_eval.py:66-67 (model rate = ST-SIM rate)
MAX_ALIGN_SHIFT = 400     # ...:77
MEL_HOP = 128             # ...:81
ROW_KEYS = ("len_samples", "psnr_global_db", "stsim_global", "psnr_masked_db", "psnr_unmasked_db", "snr_masked_db",
            "snr_unmasked_db", "mae_masked", "mae_unmasked", "stsim_masked", "stsim_unmasked")   # eval_metrics.csv after "stem"


def _backend(backend):
    if backend not in ops.SSIM_MODES:
        raise ValueError(f"backend must be 'ssim' (skimage's SSIM) or 'norm' (the reference without scikit-image), not {backend!r}")
    return backend


def frame_token_mask(latent_mask: torch.Tensor, T_wave: int) -> torch.Tensor:
    """Token mask [T_lat] -> frame mask [1 + T_wave // 128] (bool, on the mask's device): frame f belongs to token
    floor(f * 128 / (T_wave / T_lat)) computed in float64, clipped to [0, T_lat-1] (PLC/PLC1_eval.py:312-318).  All False
    when T_lat or T_wave is 0."""
    fm, _, _ = ops.frame_subsets(latent_mask, int(T_wave), 1 + int(T_wave) // MEL_HOP, MEL_HOP)
    return fm.bool()


def _stsim_device(ref_1T, est_1T, latent_mask, backend):
    """float64 [1] (global) or [3] (global, masked, unmasked) on the device: two launches after the mel front end."""
    from .losses import mel_plane
    M, maxv, nfr = mel_plane(ref_1T, est_1T)
    dev = M.device
    if latent_mask is None:
        desc = torch.tensor([[0, nfr, 0, 1, -1]], dtype=torch.int32).to(dev)
        widths = torch.full((1,), nfr, dtype=torch.int32, device=dev)
        return ops.mel_ssim(M, maxv, desc, widths, nfr, mode=backend)
    widths = torch.full((3,), nfr, dtype=torch.int32, device=dev)
    _, cols, _ = ops.frame_subsets(latent_mask, ref_1T.shape[-1], nfr, MEL_HOP, out_counts=widths[1:])
    desc = torch.tensor([[0, nfr, 0, 1, -1], [0, nfr, 0, 1, 0], [0, nfr, 0, 1, nfr]], dtype=torch.int32).to(dev)
    return ops.mel_ssim(M, maxv, desc, widths, nfr, cols=cols.reshape(-1), mode=backend)


@torch.no_grad()
def stsim_mel_with_mask(ref_1T, est_1T, latent_mask, backend: str = "ssim"):
    """compute_stsim_mel_with_mask (PLC/PLC1_eval.py:270-333) on the device -> (global, masked, unmasked) floats.  ref_1T,
    est_1T: aligned [1, T] at 24 kHz; latent_mask: [T_lat] bool.  The masked / unmasked images are the concatenated frame
    columns of each side; an empty side is NaN, a side of 1..6 frames is scored by the norm formula (the reference's
    fall-through when skimage refuses it).  backend "ssim": skimage's structural_similarity (restated);
    "norm": the reference as it runs without scikit-image.  One device->host copy."""
    _backend(backend)
    return tuple(_stsim_device(ref_1T, est_1T, latent_mask.reshape(-1), backend).cpu().tolist())


@torch.no_grad()
def stsim_mel_global(ref_1T, est_1T, backend: str = "ssim") -> float:
    """compute_stsim_mel_global (PLC/PLC1_low_mid_high_eval.py:264-288): the same score over the whole mel image."""
    _backend(backend)
    return float(_stsim_device(ref_1T, est_1T, None, backend).cpu()[0])


@torch.no_grad()
def mae_global(ref_1T, est_1T) -> float:
    """mean |r - e| (PLC/PLC1_low_mid_high_eval.py:214-217)."""
    r = ref_1T.reshape(-1).to(torch.float32); e = est_1T.reshape(-1).to(torch.float32)
    return float((r - e).abs().mean().cpu())


def _sanitize(x):
    """sanitize_wave (PLC/PLC1_eval.py:94-96)."""
    return torch.nan_to_num(x, nan=0.0, posinf=0.9999, neginf=-0.9999).clamp(-1.0, 1.0)


def _row_from(stats, stsim, T, T_lat, peak, shift):
    """The CSV row from the subset sums (ops.subset_stats) and the three ST-SIMs, on the host in float64."""
    nan, eps = float("nan"), METRIC_EPS
    pk = max(float(peak), eps)
    db = lambda num, mse: 10.0 * math.log10(num / (mse + eps))
    row = {"len_samples": int(T)}
    d2_all = stats[3] + stats[7]
    row["psnr_global_db"] = db(pk * pk, d2_all / T) if T else nan
    row["stsim_global"] = stsim[0]
    sides = {}
    for name, (c, a, r2, d2) in (("masked", stats[0:4]), ("unmasked", stats[4:8])):
        if c == 0 or T_lat == 0 or T == 0:
            sides[name] = (nan, nan, nan)
        else:
            sides[name] = (db(pk * pk, d2 / c), db(r2 / c, d2 / c), a / c)
    for name in ("masked", "unmasked"):
        row[f"psnr_{name}_db"], row[f"snr_{name}_db"], row[f"mae_{name}"] = sides[name]
    row["stsim_masked"], row["stsim_unmasked"] = stsim[1], stsim[2]
    row = {k: row[k] for k in ROW_KEYS}
    row["mae_global"] = (stats[1] + stats[5]) / T if T else nan
    row["best_shift"] = int(shift)
    return row


@torch.no_grad()
def evaluate_file(net, a_raw, asr, t_raw, tsr, peak, *, mask=None, mask_fn=None, max_shift: int = MAX_ALIGN_SHIFT,
                  backend: str = "ssim") -> dict:
    """One pass-1 iteration of PLC/PLC1_eval.py:eval_model (lines 601-663) for one file: a_raw [C, T_a] at ``asr``, t_raw
    [C, T_t] at ``tsr`` (raw amplitude), ``peak`` the global tactile peak.  Scale, resample to 24 kHz, crop to L, sanitize,
    ``net.forward_step`` (``mask`` / ``mask_fn`` as AllPredPLC takes them; default the reference's packet draw), de-normalise,
    crop, align (+-max_shift), crop, global PSNR, the three mel ST-SIMs and the six masked figures.  Returns the
    eval_metrics.csv keys after "stem" (ROW_KEYS) plus "mae_global" (PLC1_low_mid_high_eval.py's third figure) and
    "best_shift".  Two device->host copies: the alignment shift and the final row."""
    from .resample import resample_to
    _backend(backend)
    dev = next(net.predict.parameters()).device
    a_raw = a_raw.to(device=dev, dtype=torch.float32)
    t_raw = t_raw.to(device=dev, dtype=torch.float32)
    scale = t_raw.abs().amax().clamp_min(1e-8)                          # max(float(|t|.max()), 1e-8), kept on the device
    aw = resample_to(a_raw[:1], asr, TARGET_SR)                         # channels resample independently: [:1] first
    tw = resample_to(t_raw[:1] / scale, tsr, TARGET_SR)
    L = min(aw.shape[-1], tw.shape[-1])
    a_1T = _sanitize(aw[..., :L]).unsqueeze(0)
    t_1T = _sanitize(tw[..., :L]).unsqueeze(0)
    out = net.forward_step(a_1T, t_1T, mask=mask, mask_fn=mask_fn)
    ref = resample_to(t_raw[:1], tsr, TARGET_SR)
    return metrics_stage(ref, out["y_hat"][0] * scale, out["latent_mask"][0, 0], peak, max_shift, backend)


@torch.no_grad()
def metrics_stage(ref, est, latent_mask, peak, max_shift: int = MAX_ALIGN_SHIFT, backend: str = "ssim") -> dict:
    """The metric half of evaluate_file (PLC/PLC1_eval.py:628-663): ref [1, T_ref] and the de-normalised est [1, T_est] at
    24 kHz on the device, latent_mask [T_lat] -> the row.  Crop, align, crop, then two launches of subset sums and the mel
    front end + frame subsets + SSIM; two device->host copies (the shift and the row)."""
    from .proposed import align_by_xcorr, crop_match
    _backend(backend)
    lm = latent_mask.reshape(-1)
    ref_c, est_c = crop_match(ref, est)
    ref_a, est_a, shift = align_by_xcorr(ref_c, est_c, max_shift)       # device->host copy 1: the shift
    ref_a, est_a = crop_match(ref_a, est_a)
    ref_a, est_a = ref_a.contiguous(), est_a.contiguous()
    T = ref_a.shape[-1]
    stats = ops.subset_stats(ref_a, est_a, lm)
    stsim = _stsim_device(ref_a, est_a, lm, backend)
    vals = torch.cat([stats, stsim]).cpu().tolist()                    # device->host copy 2: the row
    return _row_from(vals[:8], vals[8:], T, lm.numel(), peak, shift)


def make_category_token_loss_mask(category: str, batch_size: int, T_lat: int, tokens_per_sec: float, device) -> torch.Tensor:
    """Burst loss of one fixed category (PLC/PLC1_low_mid_high_eval.py:372-418): bursts drawn with Python's ``random``
    (seed it as the reference does), host logic.  -> bool [B, T_lat]."""
    import random
    if T_lat <= 0:
        return torch.zeros(batch_size, 0, dtype=torch.bool, device=device)
    if category not in CAT_BURST_MS:
        raise ValueError(f"Unknown category: {category}")
    min_ms, max_ms = CAT_BURST_MS[category]
    nb_min, nb_max = CAT_N_BURSTS[category]
    mask = torch.zeros(batch_size, T_lat, dtype=torch.bool)
    for b in range(batch_size):
        min_tok = max(1, int(round(min_ms * tokens_per_sec / 1000.0)))
        max_tok = min(max(min_tok, int(round(max_ms * tokens_per_sec / 1000.0))), T_lat)
        for _ in range(random.randint(nb_min, nb_max)):
            L_b = random.randint(min_tok, max_tok)
            if L_b >= T_lat:
                mask[b, :] = True
                break
            s = random.randint(0, max(0, T_lat - L_b))
            mask[b, s:s + L_b] = True
    return mask.to(device)


CAT_BURST_MS = {"low": (20.0, 120.0), "medium": (120.0, 320.0), "high": (320.0, 1000.0)}   # ...low_mid_high_eval.py:88-92
CAT_N_BURSTS = {"low": (1, 2), "medium": (1, 3), "high": (1, 4)}                            # ...:95-99


def category_mask_fn(category: str):
    """mask_fn for AllPredPLC.forward_step / evaluate_file: the category model's mask with tokens_per_sec = T_lat (its
    forward_step, ...low_mid_high_eval.py:460-471)."""
    return lambda B, T_lat, device: make_category_token_loss_mask(category, B, T_lat, float(T_lat), device)
