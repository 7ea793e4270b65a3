"""Torch-CPU restatement of the training step under a lossy link (AllPredAR / AllPredPLC.forward_step with nb_valid / na_valid /
audio_conceal), built from oracle.dac24_torch's own modules (imported, not modified).  A helper, not a test.

  * masked softmax runs over the present keys only; an item (or chunk) without a key gives ctx = 0 and zero gradients there
    (filtered with ``where``: a row of -inf would give NaN);
  * the layered sum is the reference's straight-through estimator at the token's own book count, written so that the forward
    value is the RECEIVER's sum ((+0 + e_0) + e_1) + ... over the first nb_valid[b, t] books and autograd yields m * g per token:
    every kept stage adds q_i.detach() + (residual_i - residual_i.detach()) -- an exact zero whose derivative is I, as the
    reference's (q - residual).detach() + residual has;
  * qa comes from the audio codes with the stages that arrived, "hold" forward-fills lost tokens (+0 before the first
    arrival), "mask" takes them out of the keys; z_hat -- what the receiver will hold -- feeds the next chunk with gradient."""
import math
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from oracle import dac24_torch as O  # noqa: E402


def masked_attention(Q, K, V, mask, dh):
    """Q [B,H,Tq,dh], K / V [B,H,Tk,dh], mask bool [B,Tk] (True = present) or None -> ctx [B,H,Tq,dh]."""
    s = (Q @ K.transpose(-2, -1)) / math.sqrt(dh)
    if mask is None:
        return s.softmax(dim=-1) @ V
    m = mask[:, None, None, :].expand_as(s)
    has = mask.any(dim=-1)[:, None, None, None].expand_as(s)
    s = torch.where(m, s, torch.full_like(s, float("-inf")))
    s = torch.where(has, s, torch.zeros_like(s))                         # a keyless row: any finite values, dropped below
    p = torch.where(m & has, s.softmax(dim=-1), torch.zeros_like(s))
    Vz = torch.where(mask[:, None, :, None].expand_as(V), V, torch.zeros_like(V))   # an absent column's values never count
    return p @ Vz


def predictor(pr, zt_prev, za, key_mask=None):
    """O.CrossPredictor.forward with the attention under ``key_mask`` (uint8 / bool [B, Tk], nonzero = present)."""
    q = pr.ln_q(pr.pos(zt_prev).permute(0, 2, 1))
    kv = pr.ln_kv(pr.pos(za).permute(0, 2, 1))
    Q, K, V = pr._split(pr.q_proj(q)), pr._split(pr.k_proj(kv)), pr._split(pr.v_proj(kv))
    ctx = masked_attention(Q, K, V, None if key_mask is None else key_mask != 0, pr.dh)
    B, H, T, D = ctx.shape
    y = pr.out(pr.drop(ctx.permute(0, 2, 1, 3).contiguous().view(B, T, H * D)))
    y = y + q
    y = y + pr.ffn(y)
    return y.permute(0, 2, 1)


def layered_ste(vq, z, nb_valid):
    """z [B,D,T], nb_valid integer [B,T] -> (q [B,D,T], idx int64 [n_books, B, T]).  The full greedy search; the sum keeps the first
    nb_valid[b, t] stages."""
    B, D, T = z.shape
    x = z.permute(0, 2, 1).reshape(B * T, D)
    m = nb_valid.reshape(B * T).to(torch.int64)
    residual, q_sum, idx = x, torch.zeros_like(x), []
    for i, cb in enumerate(vq.books):
        emb = cb.detach()
        j = vq._nearest_l2(residual, emb)
        q = F.embedding(j, emb)
        keep = (m > i).to(x.dtype).unsqueeze(1)
        q_sum = q_sum + keep * (q.detach() + (residual - residual.detach()))
        residual = residual - q
        idx.append(j.reshape(B, T))
    return q_sum.view(B, T, D).permute(0, 2, 1).contiguous(), torch.stack(idx)


@torch.no_grad()
def audio_from_codes(quant, codes, na_valid=None):
    """qa [B,C,Ta] = the sum, in stage order, of out_proj_i(codebook_i[codes_i]) over the stages that arrived."""
    qa = 0
    for i, q in enumerate(quant.quantizers[:codes.shape[1]]):
        z_i = q.out_proj(F.embedding(codes[:, i], q.codebook.weight).transpose(1, 2))
        if na_valid is not None:
            z_i = z_i * (na_valid.to(torch.int64) > i).to(z_i.dtype).unsqueeze(1)
        qa = qa + z_i
    return qa


@torch.no_grad()
def hold_fill(qa, na_valid):
    out = qa.clone()
    B, C, T = qa.shape
    for b in range(B):
        last = torch.zeros(C, dtype=qa.dtype)
        for t in range(T):
            if int(na_valid[b, t]) != 0:
                last = qa[b, :, t]
            else:
                out[b, :, t] = last
    return out


def audio_side(ref, a, na_valid, audio_conceal):
    """-> (qa, key_mask or None, codes) as the receiver reconstructs the audio latents."""
    with torch.no_grad():
        qa, codes, *_ = ref.A_QUANT(ref.A_ENC(a))
        if na_valid is not None:
            qa = audio_from_codes(ref.A_QUANT, codes, na_valid)
            if audio_conceal == "hold":
                qa = hold_fill(qa, na_valid)
    return qa, (na_valid if (audio_conceal == "mask" and na_valid is not None) else None), codes


def forward_step_link(ref, a, tc, nb_valid=None, na_valid=None, audio_conceal="zero"):
    """O.ProposedEval.forward_step under the link -> its keys plus "z_run", "idx", "codes"."""
    Tw = tc.shape[-1]
    qa, key_mask, codes = audio_side(ref, a, na_valid, audio_conceal)
    with torch.no_grad():
        zt = ref.T_ENC(tc)
    B, C, Tlat = zt.shape
    nbv = nb_valid if nb_valid is not None else torch.full((B, Tlat), len(ref.vq.books), dtype=torch.uint8)
    chunks, rD_all, idx_all, last = [], [], [], None
    for s in range(0, Tlat, ref.chunk):
        e = min(Tlat, s + ref.chunk)
        zt_prev = zt.new_zeros(B, C, e - s)
        if last is not None:
            zt_prev = torch.cat([last, zt_prev[..., 1:]], dim=-1)                 # column 0 <- z_run[..., s-1], with graph
        km = key_mask[:, s:e] if key_mask is not None else None
        z_pred = predictor(ref.predict, zt_prev, qa[..., s:e], km)
        r = zt[..., s:e] - z_pred.detach()
        rN = torch.tanh(ref.tokennorm(r))
        rD = ref.proj_down(ref.scale.clamp(5e-3, 0.5) * rN)
        qD, idx = layered_ste(ref.vq, rD, nbv[:, s:e])
        z_hat = z_pred + ref.proj_up(qD)
        chunks.append(z_hat)
        rD_all.append(rD)
        idx_all.append(idx)
        last = z_hat[..., -1:]
    z_run = torch.cat(chunks, dim=-1)
    y_hat = ref.T_DEC(z_run)
    T = min(y_hat.shape[-1], tc.shape[-1], Tw)
    return {"y_hat": y_hat[..., :T], "tgt": tc[..., :T], "r_tokens": torch.cat([r.detach() for r in rD_all], dim=-1), "z_run": z_run,
            "idx": torch.cat(idx_all, dim=-1), "codes": codes, "rD": rD_all}


def plc_step_link(ref, a, tc, lost, na_valid, audio_conceal):
    """AllPredPLC.forward_step's arithmetic on ref's backbones and predictor (PLC/PLC1.py:401-410) with the audio side under loss:
    lost bool [B, T_lat] -> {"y_hat", "tgt"}."""
    Tw = tc.shape[-1]
    qa, key_mask, _ = audio_side(ref, a, na_valid, audio_conceal)
    with torch.no_grad():
        zt = ref.T_ENC(tc)
    zt_in = zt * (~lost).unsqueeze(1)
    z_pred = predictor(ref.predict, zt_in, qa, key_mask)
    y_hat = ref.T_DEC(torch.where(lost.unsqueeze(1), z_pred, zt_in))
    T = min(y_hat.shape[-1], tc.shape[-1], Tw)
    return {"y_hat": y_hat[..., :T], "tgt": tc[..., :T]}
