"""CPU restatement of the receiver's audio concealment (decode_latents(audio_conceal=...)), from numpy
copies and the oracle's own pieces (orc.layernorm_c, orc.conv1d through orc._linear, orc.attention, orc.gelu) and the loops of
tests/lossy_oracle.py / tests/av_oracle.py.  Shared by tests/test_audio_conceal_cpu.py and tests/test_gpu_audio_conceal.py.

  * hold_fill: y[b, c, t] = x[b, c, s(b, t)], s(b, t) the largest t' <= t with valid[b, t'] != 0, else carry[b, c] (+0 without);
    pure copies; -> (y, the carry after the call = y[..., T-1]);
  * masked_cross_predictor: orc.cross_predictor with the attention run per item on the columns J(b) of K and V (ascending list of
    the present keys); everything before and after the attention is per token and does not see the mask;
  * masked_loop / masked_two_pass: lossy_oracle's two orders with that predictor;
  * receiver_av_conceal: av_oracle.receiver_av under a mode;
  * audio_loss / check_audio_loss: the loss patterns of the end-to-end tests and the conditions they state."""
import numpy as np

import av_oracle as av
import lossy_oracle as lo
import receiver_oracle as ro

CHUNK = lo.CHUNK
MODES = ("zero", "mask", "hold")


def hold_fill(x, valid, carry=None):
    """x[B, C, T], valid[B, T], carry[B, C] or None -> (y[B, C, T], carry_out[B, C]).  np.where copies bits."""
    x = np.asarray(x, np.float32)
    B, C, T = x.shape
    last = np.zeros((B, C), np.float32) if carry is None else np.array(carry, np.float32, copy=True)
    y = np.empty_like(x)
    ok = np.asarray(valid) != 0
    for t in range(T):
        last = np.where(ok[:, t, None], x[:, :, t], last)
        y[:, :, t] = last
    return y, last


def masked_attention(orc, Q, K, V, mask, heads):
    """Per item b: orc.attention on K, V compacted to the columns with mask[b, j] != 0."""
    ctx = np.zeros_like(Q)
    for b in range(Q.shape[0]):
        J = np.flatnonzero(np.asarray(mask[b]) != 0)
        ctx[b:b + 1] = orc.attention(Q[b:b + 1], np.ascontiguousarray(K[b:b + 1][:, :, J]), np.ascontiguousarray(V[b:b + 1][:, :, J]),
                                     heads)
    return ctx


def masked_cross_predictor(orc, sd, zt_prev, za, pe, mask, heads=8, prefix="predict."):
    """oracle.cross_predictor with a key mask[B, Tk] (nonzero = present)."""
    P = prefix
    zt_prev = np.asarray(zt_prev, np.float32); za = np.asarray(za, np.float32)
    Tq, Tk = zt_prev.shape[2], za.shape[2]
    assert tuple(np.asarray(mask).shape) == (za.shape[0], Tk)
    q = orc.layernorm_c(zt_prev + pe[:Tq].T[None], sd[P + "ln_q.weight"], sd[P + "ln_q.bias"])
    kv = orc.layernorm_c(za + pe[:Tk].T[None], sd[P + "ln_kv.weight"], sd[P + "ln_kv.bias"])
    Q = orc._linear(q, sd[P + "q_proj.weight"])
    K = orc._linear(kv, sd[P + "k_proj.weight"])
    V = orc._linear(kv, sd[P + "v_proj.weight"])
    ctx = masked_attention(orc, Q, K, V, mask, heads)
    y1 = orc._linear(ctx, sd[P + "out.weight"], residual=q)
    h = orc.layernorm_c(y1, sd[P + "ffn.0.weight"], sd[P + "ffn.0.bias"])
    h = orc.gelu(orc._linear(h, sd[P + "ffn.1.weight"], sd[P + "ffn.1.bias"]))
    return orc._linear(h, sd[P + "ffn.3.weight"], sd[P + "ffn.3.bias"], residual=y1)


def masked_loop(orc, sd, qa, idx, nb_valid, mask, books_use=None):
    """lossy_oracle.lossy_loop with the key mask[B, Ta] on the predictor."""
    qD = lo.dequant_layers(ro.books_of(sd), idx, nb_valid, books_use)
    B, _, Tlat = qD.shape
    C = np.asarray(sd["proj_up.weight"]).shape[0]
    pe = ro._pe(orc, sd)
    mask = np.asarray(mask)
    z_run = np.zeros((B, C, Tlat), np.float32)
    for s in range(0, Tlat, CHUNK):
        e = min(Tlat, s + CHUNK)
        zt_prev = np.zeros((B, C, e - s), np.float32)
        if s == 0:
            zt_prev[..., 1:] = z_run[..., s:e - 1]
        else:
            zt_prev[...] = z_run[..., s - 1:e - 1]
        z_pred = masked_cross_predictor(orc, sd, zt_prev, qa[..., s:e], pe, mask[:, s:e])
        z_run[..., s:e] = ro._proj_up(orc, sd, qD[..., s:e], residual=z_pred)
    return z_run


def masked_two_pass(orc, sd, qa, idx, nb_valid, mask, books_use=None):
    """lossy_oracle.lossy_two_pass with the key mask: the mask touches K / V alone, which do not depend on the loop."""
    qD = lo.dequant_layers(ro.books_of(sd), idx, nb_valid, books_use)
    B, _, Tlat = qD.shape
    C = np.asarray(sd["proj_up.weight"]).shape[0]
    pe = ro._pe(orc, sd)
    mask = np.asarray(mask)
    starts = list(range(0, Tlat, CHUNK))
    nt = {s: min(Tlat, s + CHUNK) - s for s in starts}
    ka = {s: qa[..., s:s + nt[s]].shape[-1] for s in starts}

    def grouped(chunks, tq_of, zt_of):
        out = {}
        for key in sorted({(tq_of(s), ka[s]) for s in chunks}):
            grp = [s for s in chunks if (tq_of(s), ka[s]) == key]
            zt = np.concatenate([zt_of(s) for s in grp], axis=0)
            za = np.concatenate([qa[..., s:s + key[1]] for s in grp], axis=0)
            mk = np.concatenate([mask[:, s:s + key[1]] for s in grp], axis=0)
            zp = masked_cross_predictor(orc, sd, zt, za, pe, mk)
            for j, s in enumerate(grp):
                out[s] = zp[j * B:(j + 1) * B]
        return out

    p1 = grouped(starts, lambda s: nt[s], lambda s: np.zeros((B, C, nt[s]), np.float32))
    z_run = ro._proj_up(orc, sd, qD, residual=np.concatenate([p1[s] for s in starts], axis=-1))
    later = starts[1:]
    p2 = grouped(later, lambda s: 1, lambda s: np.ascontiguousarray(z_run[..., s - 1:s]))
    for s in later:
        z_run[..., s:s + 1] = ro._proj_up(orc, sd, np.ascontiguousarray(qD[..., s:s + 1]), residual=p2[s])
    return z_run


def conceal_qa(orc, q3, codes, na_valid, mode, carry=None):
    """-> (qa the predictor is fed, key mask or None, the hold carry after the call or None)."""
    qa = av.from_codes_layers(orc, *q3, codes, na_valid)
    if mode == "hold":
        qa, carry = hold_fill(qa, np.asarray(na_valid) != 0, carry)
        return qa, None, carry
    return qa, ((np.asarray(na_valid) != 0) if mode == "mask" else None), None


def receiver_av_conceal(orc, sd, q3, codes, idx, nb_valid, na_valid, mode):
    """av_oracle.receiver_av under audio_conceal = mode, on lossy_oracle.lossy_loop's loop."""
    assert mode in MODES
    qa, mask, _ = conceal_qa(orc, q3, codes, na_valid, mode)
    if mask is None:
        return lo.lossy_loop(orc, sd, qa, idx, nb_valid)
    return masked_loop(orc, sd, qa, idx, nb_valid, mask)


# ------------------------------------------------------------------------------------------------------------ loss patterns
def audio_loss(B, Ta, na=32, packet_tok=2, kinds=None):
    """na_valid uint8 [B, Ta] of the end-to-end tests (packets of ``packet_tok`` tokens).  Item b is of kind kinds[b] (default
    b % 3): kind 0 loses nothing; kind 1 loses token 0 (its first packet) and all of chunk 1; kind 2 loses every other packet and
    the last token."""
    kinds = [b % 3 for b in range(B)] if kinds is None else list(kinds)
    v = np.full((B, Ta), na, np.uint8)
    P = (Ta + packet_tok - 1) // packet_tok
    for b in range(B):
        if kinds[b] == 1:
            v[b, :packet_tok] = 0
            v[b, CHUNK:2 * CHUNK] = 0
        elif kinds[b] == 2:
            for p in range(1, P, 2):
                v[b, p * packet_tok:(p + 1) * packet_tok] = 0
            v[b, (P - 1) * packet_tok:] = 0
    return v


def check_audio_loss(v, packet_tok=2, kinds=None):
    """The conditions audio_loss states, asserted on ``v``."""
    B, Ta = v.shape
    kinds = [b % 3 for b in range(B)] if kinds is None else list(kinds)
    P = (Ta + packet_tok - 1) // packet_tok
    for b in range(B):
        row = v[b]
        lostp = [bool((row[p * packet_tok:(p + 1) * packet_tok] == 0).all()) for p in range(P)]
        for p in range(P):                                                    # packet granularity: a packet is lost whole
            assert len(set(row[p * packet_tok:(p + 1) * packet_tok].tolist())) == 1
        if kinds[b] == 0:
            assert not any(lostp)
        elif kinds[b] == 1:
            assert row[0] == 0 and (row[CHUNK:2 * CHUNK] == 0).all()
            assert (row[packet_tok:min(Ta, CHUNK)] != 0).all() and (row[2 * CHUNK:] != 0).all()
        else:
            assert row[Ta - 1] == 0 and row[0] != 0
            assert all(lostp[1::2]) and not any(lostp[0:P - 1:2])
