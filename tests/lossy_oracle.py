"""CPU restatement of the lossy-channel receiver (decode_latents(nb_valid=...)), from the pieces of tests/receiver_oracle.py
(dequant's arithmetic, _proj_up, _pe, books_of) and orc.cross_predictor.  Shared by tests/test_lossy_cpu.py and
tests/test_gpu_lossy.py.

The only difference from receiver_oracle is qD: token (b, t) sums its first min(books_use, nb_valid[b, t]) books, from +0 in book
order; a token with nb_valid == 0 (lost) has qD = 0, so z_hat = proj_up(0) + z_pred.  Indices at or above a token's count are
never looked at."""
import numpy as np

import receiver_oracle as ro

CHUNK = ro.CHUNK
PACKET_TOK = 2


def dequant_layers(books, idx, nb_valid, books_use=None):
    """idx[nb, B, T], nb_valid[B, T] -> qD[B, D, T] over the first min(nb_use, nb_valid[b, t]) books of each token."""
    idx = np.asarray(idx, np.int64)
    nbv = np.asarray(nb_valid).astype(np.int64)
    nb = min(idx.shape[0], len(books)) if books_use is None else max(0, min(int(books_use), idx.shape[0], len(books)))
    _, B, T = idx.shape
    D = books[0].shape[1]
    K = books[0].shape[0]
    q = np.zeros((B, T, D), np.float32)
    for i in range(nb):
        have = nbv > i
        rows = books[i][np.where(have, np.clip(idx[i], 0, K - 1), 0)]         # indices of absent books are not looked at
        q = np.where(have[..., None], q + rows, q)
    return np.ascontiguousarray(q.transpose(0, 2, 1))


def lossy_loop(orc, sd, qa, idx, nb_valid, books_use=None, tactile_only=False):
    """The per-chunk receiver loop (receiver_oracle.receiver_loop) on the lossy qD."""
    qD = dequant_layers(ro.books_of(sd), idx, nb_valid, books_use)
    B, _, Tlat = qD.shape
    C = np.asarray(sd["proj_up.weight"]).shape[0]
    pe = ro._pe(orc, sd)
    z_run = np.zeros((B, C, Tlat), np.float32)
    for s in range(0, Tlat, CHUNK):
        e = min(Tlat, s + CHUNK)
        zt_prev = np.zeros((B, C, e - s), np.float32)
        if s == 0:
            zt_prev[..., 1:] = z_run[..., s:e - 1]
        else:
            zt_prev[...] = z_run[..., s - 1:e - 1]
        z_pred = None if tactile_only else orc.cross_predictor(sd, zt_prev, qa[..., s:e], pe)
        z_run[..., s:e] = ro._proj_up(orc, sd, qD[..., s:e], residual=z_pred)
    return z_run


def lossy_two_pass(orc, sd, qa, idx, nb_valid, books_use=None):
    """The two-pass order (receiver_oracle.receiver_two_pass) on the lossy qD: pass 2 reads z_run[s-1], the LAST token of a full
    chunk, which is never position 0 and so does not depend on the loop, whatever was lost."""
    qD = dequant_layers(ro.books_of(sd), idx, nb_valid, books_use)
    B, _, Tlat = qD.shape
    C = np.asarray(sd["proj_up.weight"]).shape[0]
    pe = ro._pe(orc, sd)
    starts = list(range(0, Tlat, CHUNK))
    shape = {s: (min(Tlat, s + CHUNK) - s, qa[..., s:s + CHUNK][..., :min(Tlat, s + CHUNK) - s].shape[-1]) for s in starts}

    def grouped(chunks, tq_of, zt_of):
        out = {}
        for key in sorted({(tq_of(s), shape[s][1]) for s in chunks}):
            grp = [s for s in chunks if (tq_of(s), shape[s][1]) == key]
            zt = np.concatenate([zt_of(s) for s in grp], axis=0)
            za = np.concatenate([qa[..., s:s + key[1]] for s in grp], axis=0)
            zp = orc.cross_predictor(sd, zt, za, pe)
            for j, s in enumerate(grp):
                out[s] = zp[j * B:(j + 1) * B]
        return out

    p1 = grouped(starts, lambda s: shape[s][0], lambda s: np.zeros((B, C, shape[s][0]), np.float32))
    z_pred = np.concatenate([p1[s] for s in starts], axis=-1)
    z_run = ro._proj_up(orc, sd, qD, residual=z_pred)
    later = starts[1:]
    p2 = grouped(later, lambda s: 1, lambda s: np.ascontiguousarray(z_run[..., s - 1:s]))
    for s in later:
        z_run[..., s:s + 1] = ro._proj_up(orc, sd, np.ascontiguousarray(qD[..., s:s + 1]), residual=p2[s])
    return z_run


PATTERNS = ("none", "all", "tok15", "tok16", "tail_packet", "alternating", "thin1")


def loss_pattern(name, B, Tlat, nb, packet_tok=PACKET_TOK):
    """nb_valid uint8 [B, Tlat] of a named loss pattern (packets of ``packet_tok`` tokens, the same for every item)."""
    v = np.full((B, Tlat), nb, np.uint8)
    P = (Tlat + packet_tok - 1) // packet_tok
    if name == "none":
        pass
    elif name == "all":
        v[:] = 0
    elif name in ("tok15", "tok16"):                     # the last token of chunk 0 (what pass 2 reads) / position 0 of chunk 1
        t = int(name[3:])
        if t < Tlat:
            v[:, t] = 0
    elif name == "tail_packet":
        v[:, (P - 1) * packet_tok:] = 0
    elif name == "alternating":
        for p in range(1, P, 2):
            v[:, p * packet_tok:(p + 1) * packet_tok] = 0
    elif name == "thin1":
        v[:] = min(1, nb)
    else:
        raise ValueError(name)
    return v
