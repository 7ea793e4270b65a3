"""CPU restatement of the receiver (ProposedEval.decode_latents), assembled from existing oracle pieces only: orc.cross_predictor,
orc.conv1d and numpy float32 additions (exact IEEE).  Shared by tests/test_receiver_cpu.py and tests/test_gpu_receiver.py.

The receiver's arithmetic contract (include/mvq.h, mvq_rvq_dequant_f32 / mvq_dac_rvq_from_codes_f32):
  * qD = ((+0 + e_0[idx_0]) + e_1[idx_1]) + ...  in book order;
  * qa = ((0 + zq_0) + zq_1) + ...,  zq_i = out_proj_i(codebook_i[code_i]) (orc.conv1d, k = 1: fma chain over the 8 code dims,
    then + bias);
  * the transmitter's chunk loop without T_ENC / TokenNorm / proj_down / search: z_hat = proj_up(qD) + z_pred."""
import numpy as np

CHUNK = 16

# Worst |z_run(receiver) - z_run(transmitter)| / max|z_run(transmitter)| measured on the CPU by
# tests/test_receiver_cpu.py::test_restatement_against_transmitter over the two G4 cases: 6.06e-7 (b8_k512) and 7.22e-7
# (b3_k128_use2).  The GPU tests allow 10x the worst.
RX_VS_TX_MEASURED = 7.3e-7
RX_VS_TX_REL = 10 * RX_VS_TX_MEASURED

# The G4 fixture's transmitted codes (made by the reference's own classes) decoded by this restatement, against G4's z_run / y /
# PSNR, measured by tests/test_receiver_cpu.py::test_g4_codes_through_the_restatement: worst relative z_run difference 1.48e-6
# (b3_k128_use2), worst |y - y_G4| 1.26e-5 (b8_k512), worst PSNR difference 1.45e-6 dB (b8_k512).  The GPU path equals this
# restatement bit for bit; tests/test_gpu_receiver.py allows 10x each.
G4_Z_MEASURED, G4_Y_MEASURED, G4_PSNR_MEASURED = 1.5e-6, 1.27e-5, 1.5e-6
G4_Z_REL, G4_Y_ATOL, G4_PSNR_DB = 10 * G4_Z_MEASURED, 10 * G4_Y_MEASURED, 10 * G4_PSNR_MEASURED


def books_of(sd):
    books = []
    while f"vq.books.{len(books)}" in sd:
        books.append(np.asarray(sd[f"vq.books.{len(books)}"], np.float32))
    return books


def dequant(books, idx, books_use=None):
    """idx[nb, B, T] -> qD[B, D, T]."""
    idx = np.asarray(idx, np.int64)
    nb = min(idx.shape[0], len(books)) if books_use is None else max(0, min(int(books_use), idx.shape[0], len(books)))
    _, B, T = idx.shape
    D = books[0].shape[1]
    q = np.zeros((B, T, D), np.float32)
    for i in range(nb):
        q = q + books[i][idx[i]]
    return np.ascontiguousarray(q.transpose(0, 2, 1))


def from_codes(orc, sd, codes, prefix="A_QUANT."):
    """upstream ResidualVectorQuantize.from_codes -> (z_q [B,C,T], z_p [B,nq*8,T])."""
    codes = np.asarray(codes, np.int64)
    B, nq, T = codes.shape
    zq, zp = None, []
    for i in range(nq):
        p = f"{prefix}quantizers.{i}"
        cb = np.asarray(sd[p + ".codebook.weight"], np.float32)
        z_p = np.ascontiguousarray(cb[codes[:, i]].transpose(0, 2, 1))             # raw rows [B, 8, T]
        w, b = orc._wn(sd, p + ".out_proj")
        zq_i = orc.conv1d(z_p, w, b)
        zq = np.zeros_like(zq_i) + zq_i if zq is None else zq + zq_i
        zp.append(z_p)
    return zq, np.concatenate(zp, axis=1)


def _pe(orc, sd):
    return np.asarray(sd["predict.pos.pe"], np.float32) if "predict.pos.pe" in sd else orc.pos_table(1024)


def _proj_up(orc, sd, qD, residual=None):
    return orc.conv1d(qD, np.asarray(sd["proj_up.weight"], np.float32), sd["proj_up.bias"], residual=residual)


def receiver_loop(orc, sd, qa, idx, books_use=None, tactile_only=False):
    """The per-chunk receiver loop (oracle.proposed_encode_latents with the encoder side removed)."""
    qD = dequant(books_of(sd), idx, books_use)
    B, _, Tlat = qD.shape
    C = np.asarray(sd["proj_up.weight"]).shape[0]
    pe = _pe(orc, sd)
    z_run = np.zeros((B, C, Tlat), np.float32)
    for s in range(0, Tlat, CHUNK):
        e = min(Tlat, s + CHUNK)
        zt_prev = np.zeros((B, C, e - s), np.float32)
        if s == 0:
            zt_prev[..., 1:] = z_run[..., s:e - 1]
        else:
            zt_prev[...] = z_run[..., s - 1:e - 1]
        z_pred = None if tactile_only else orc.cross_predictor(sd, zt_prev, qa[..., s:e], pe)
        z_run[..., s:e] = _proj_up(orc, sd, qD[..., s:e], residual=z_pred)
    return z_run


def receiver_two_pass(orc, sd, qa, idx, books_use=None):
    """The two-pass order of decode_latents: pass 1 runs every chunk with a zero query input (chunks of one (n, ka) shape stacked
    along the batch axis), pass 2 recomputes position 0 of every chunk s > 0 from z_run[s-1] (one query per chunk, again
    stacked).  Bit-equal to receiver_loop when only column 0 of a chunk depends on the loop."""
    qD = dequant(books_of(sd), idx, books_use)
    B, _, Tlat = qD.shape
    C = np.asarray(sd["proj_up.weight"]).shape[0]
    pe = _pe(orc, sd)
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
    z_run = _proj_up(orc, sd, qD, residual=z_pred)
    later = starts[1:]
    p2 = grouped(later, lambda s: 1, lambda s: np.ascontiguousarray(z_run[..., s - 1:s]))
    for s in later:
        z_run[..., s:s + 1] = _proj_up(orc, sd, np.ascontiguousarray(qD[..., s:s + 1]), residual=p2[s])
    return z_run
