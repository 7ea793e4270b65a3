"""CPU restatement of closed-loop sender rate control (include/mvq.h: mvq_rvq_rate_f32), from numpy float32
operations (each one IEEE fp32 operation) and the pieces of tests/receiver_oracle.py, tests/lossy_oracle.py and
tests/sender_oracle.py.  Shared by tests/test_rate_cpu.py and tests/test_gpu_rate.py.

  * energies: r_0 = rD, r_{m+1} = r_m - e_m[idx_m]; E_m = (...((+0 + r_m[0]*r_m[0]) + r_m[1]*r_m[1]) + ...), d ascending, the
    multiply and the add rounded separately;
  * decide: the book count of each packet of one item from its E (constant quality: tol2; constant rate: budget);
  * rate_chunk: energies + decide + the receiver's sum over each token's count (lossy_oracle.dequant_layers);
  * closed_loop_ar: the sender's chunk loop (sender_oracle.ar_chunk) with rate_chunk's qD in place of the straight-through sum.
"""
import numpy as np

import lossy_oracle as lo
import receiver_oracle as ro

CHUNK = ro.CHUNK
f32 = np.float32


def energies(rD, books, idx, nb_use=None):
    """rD[B, D, T], books (sequence of [K, D]), idx[nb, B, T] -> (E float32 [nb_use + 1, B, T], the final residual [B, T, D])."""
    rD = np.asarray(rD, f32)
    idx = np.asarray(idx, np.int64)
    nb = min(idx.shape[0], len(books)) if nb_use is None else max(0, min(int(nb_use), idx.shape[0], len(books)))
    B, D, T = rD.shape
    r = np.ascontiguousarray(rD.transpose(0, 2, 1))
    E = np.zeros((nb + 1, B, T), f32)
    for m in range(nb + 1):
        e = np.zeros((B, T), f32)                                       # +0
        for d in range(D):
            e = e + r[..., d] * r[..., d]                               # two float32 operations, d ascending
        E[m] = e
        if m < nb:
            bk = np.asarray(books[m], f32)
            r = r - bk[np.clip(idx[m], 0, bk.shape[0] - 1)]
    return E, r


def decide(E, rate, packet_tok, group_tok=CHUNK):
    """E[nb + 1, T] of ONE item -> nb_sent int64 [P]: the books of each packet under ``rate`` (a packets.Rate)."""
    E = np.asarray(E, f32)
    nb, T = E.shape[0] - 1, E.shape[1]
    min_books, mode, tol2, budget = rate.resolve(nb, packet_tok, group_tok)
    tol2 = f32(tol2)
    P = (T + packet_tok - 1) // packet_tok
    pc = group_tok // packet_tok
    out = np.zeros(P, np.int64)
    if nb == 0:
        return out
    toks = lambda p: range(p * packet_tok, min(T, (p + 1) * packet_tok))
    for g0 in range(0, P, pc):
        pk = list(range(g0, min(P, g0 + pc)))
        if mode == 0:
            out[pk] = nb
        elif mode == 1:
            for p in pk:
                need_max = min_books
                for j in toks(p):
                    thr = tol2 * E[0, j]                                # one fp32 multiply
                    need = nb
                    for m in range(min_books, nb + 1):
                        if E[m, j] <= thr:                              # a NaN comparison is false
                            need = m
                            break
                    need_max = max(need_max, need)
                out[p] = need_max
        else:
            g = len(pk)
            left = max(g * min_books, (budget * g) // pc) - g * min_books
            m_of = {p: min_books for p in pk}

            def gain(p):
                s = f32(0.0)
                for j in toks(p):
                    s = f32(s + f32(E[m_of[p], j] - E[m_of[p] + 1, j]))
                return s

            while left > 0:
                win, gw = None, None
                for p in pk:                                            # ascending packet order
                    if m_of[p] >= nb:
                        continue
                    gp = gain(p)
                    if win is None or gp > gw:                          # strictly greater: lowest index on ties, a NaN never displaces
                        win, gw = p, gp
                if win is None:
                    break
                m_of[win] += 1
                left -= 1
            for p in pk:
                out[p] = m_of[p]
    return out


def expand(nb_sent, T, packet_tok):
    """nb_sent[..., P] -> nb_valid uint8 [..., T]: a token has its packet's count."""
    return np.repeat(np.asarray(nb_sent), packet_tok, axis=-1)[..., :T].astype(np.uint8)


def rate_chunk(rD, books, idx, rate, packet_tok, nb_use=None, group_tok=CHUNK):
    """-> (qD[B, D, T] the receiver's sum over each token's count, nb_valid uint8 [B, T], nb_sent uint8 [B, P], E[nb + 1, B, T])."""
    E, _ = energies(rD, books, idx, nb_use)
    B, _, T = np.asarray(rD).shape
    nb_sent = np.stack([decide(E[:, b], rate, packet_tok, group_tok) for b in range(B)]).astype(np.uint8)
    nb_valid = expand(nb_sent, T, packet_tok)
    return lo.dequant_layers(books, idx, nb_valid, E.shape[0] - 1), nb_valid, nb_sent, E


def closed_loop_ar(orc, sd, qa, zt, rate, packet_tok=lo.PACKET_TOK, books_use=None):
    """The sender's AR loop, closed: per chunk the search on rD, then rate_chunk's qD -- the receiver's sum over the books each
    packet carries -- in place of the straight-through sum.  ``qa``: the audio latent the RECEIVER has (from the codes).
    -> (z_run, idx[nb, B, Tlat], nb_valid uint8 [B, Tlat], nb_sent uint8 [B, P], rD[B, D, Tlat])."""
    B, C, Tlat = zt.shape
    pe = ro._pe(orc, sd)
    books = ro.books_of(sd)
    scale = f32(min(max(float(f32(sd["scale"])), 5e-3), 0.5))
    z_run = np.zeros((B, C, Tlat), f32)
    ids, nbv, nbs, rDs = [], [], [], []
    for s in range(0, Tlat, CHUNK):
        e = min(Tlat, s + CHUNK)
        n = e - s
        zt_prev = np.zeros((B, C, n), f32)
        if s > 0:
            zt_prev[..., 0] = z_run[..., s - 1]
        z_pred = orc.cross_predictor(sd, zt_prev, np.ascontiguousarray(qa[..., s:e]), pe)
        rN = orc.layernorm_c(np.ascontiguousarray(zt[..., s:e]) - z_pred, sd["tokennorm.ln.weight"], sd["tokennorm.ln.bias"],
                             do_tanh=True, post_scale=scale)
        rD = orc.conv1d(rN, np.asarray(sd["proj_down.weight"], f32), sd["proj_down.bias"])
        _, idx = orc.rvq_ema_forward(rD, books, books_use)
        idx = idx.reshape(idx.shape[0], B, n)
        qD, v, c, _ = rate_chunk(rD, books, idx, rate, packet_tok)
        z_run[..., s:e] = ro._proj_up(orc, sd, qD, residual=z_pred)
        ids.append(idx); nbv.append(v); nbs.append(c); rDs.append(rD)
    cat = lambda xs: np.concatenate(xs, axis=-1)
    return z_run, cat(ids), cat(nbv), cat(nbs), cat(rDs)


def real_rD(orc, sd, B, T, seed):
    """A code-domain residual as the AR loop's first chunk sees it: seeded zt / qa through the predictor, TokenNorm and proj_down
    (T <= 16 per call of the predictor; longer T is built chunk by chunk with a zero shift-by-one input)."""
    r = np.random.default_rng(seed)
    C = np.asarray(sd["proj_up.weight"]).shape[0]
    zt = (0.5 * r.standard_normal((B, C, T))).astype(f32)
    qa = (0.5 * r.standard_normal((B, C, T))).astype(f32)
    pe = ro._pe(orc, sd)
    scale = f32(min(max(float(f32(sd["scale"])), 5e-3), 0.5))
    out = []
    for s in range(0, T, CHUNK):
        e = min(T, s + CHUNK)
        z_pred = orc.cross_predictor(sd, np.zeros((B, C, e - s), f32), np.ascontiguousarray(qa[..., s:e]), pe)
        rN = orc.layernorm_c(np.ascontiguousarray(zt[..., s:e]) - z_pred, sd["tokennorm.ln.weight"], sd["tokennorm.ln.bias"],
                             do_tanh=True, post_scale=scale)
        out.append(orc.conv1d(rN, np.asarray(sd["proj_down.weight"], f32), sd["proj_down.bias"]))
    return np.concatenate(out, axis=-1)
