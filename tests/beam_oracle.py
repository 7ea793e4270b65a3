"""The C restatement of the sender's beam search (tests/beam_ref/rvq_beam_ref.c; include/mvq.h: mvq_rvq_beam_f32; DESIGN.md section
33), built with the oracle's flags into a directory the caller names, and the closed loop of tests/rate_oracle.py with the beam in
place of the greedy search.  Shared by tests/test_beam_cpu.py and tests/test_gpu_beam.py."""
import ctypes
import subprocess
from pathlib import Path

import numpy as np

import lossy_oracle as lo
import rate_oracle as rt
import receiver_oracle as ro

ROOT = Path(__file__).resolve().parent.parent
f32 = np.float32


def build(out_dir):
    """-> search(rD[B, D, T], books (sequence of [K, D]), beam, nb_use=None) -> (idx int32 [nb, B*T], slot uint8 [B*T], energy
    float32 [B*T])."""
    out = Path(out_dir) / "libbeamref.so"
    subprocess.run(["gcc", "-O3", "-mavx2", "-mfma", "-ffp-contract=off", "-fno-math-errno", "-fPIC", "-Wall", "-shared", "-o", str(out),
                    str(ROOT / "tests" / "beam_ref" / "rvq_beam_ref.c"), "-lm"], check=True, capture_output=True)
    lib = ctypes.CDLL(str(out))
    fp = ctypes.POINTER(ctypes.c_float)
    lib.ref_rvq_beam.argtypes = [fp, fp, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint8), fp] + [ctypes.c_int] * 6
    lib.ref_rvq_beam.restype = ctypes.c_int

    def search(rD, books, beam, nb_use=None):
        rD = np.ascontiguousarray(rD, f32)
        B, D, T = rD.shape
        nb = len(books) if nb_use is None else max(0, min(int(nb_use), len(books)))
        bk = np.ascontiguousarray(np.stack([np.asarray(b, f32) for b in books[:nb]])) if nb else np.zeros((0, 1, D), f32)
        K = bk.shape[1]
        idx = np.full((nb, B * T), -7, np.int32)
        slot = np.full(B * T, 0xEE, np.uint8)
        energy = np.full(B * T, -1.0, f32)
        rc = lib.ref_rvq_beam(rD.ctypes.data_as(fp), bk.ctypes.data_as(fp), idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                              slot.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), energy.ctypes.data_as(fp), B, D, T, nb, K, int(beam))
        assert rc == 0, rc
        return idx, slot, energy
    return search


def closed_loop_ar_beam(search, orc, sd, qa, zt, rate, packet_tok=lo.PACKET_TOK, books_use=None):
    """rate_oracle.closed_loop_ar with ``search`` (beam = rate.beam) where it runs the greedy search: the pieces are rate_oracle's and
    receiver_oracle's own.  -> (z_run, idx[nb, B, Tlat], nb_valid uint8 [B, Tlat], nb_sent uint8 [B, P], rD[B, D, Tlat])."""
    B, C, Tlat = zt.shape
    pe = ro._pe(orc, sd)
    books = ro.books_of(sd)
    scale = f32(min(max(float(f32(sd["scale"])), 5e-3), 0.5))
    z_run = np.zeros((B, C, Tlat), f32)
    ids, nbv, nbs, rDs = [], [], [], []
    for s in range(0, Tlat, rt.CHUNK):
        e = min(Tlat, s + rt.CHUNK)
        n = e - s
        zt_prev = np.zeros((B, C, n), f32)
        if s > 0:
            zt_prev[..., 0] = z_run[..., s - 1]
        z_pred = orc.cross_predictor(sd, zt_prev, np.ascontiguousarray(qa[..., s:e]), pe)
        rN = orc.layernorm_c(np.ascontiguousarray(zt[..., s:e]) - z_pred, sd["tokennorm.ln.weight"], sd["tokennorm.ln.bias"],
                             do_tanh=True, post_scale=scale)
        rD = orc.conv1d(rN, np.asarray(sd["proj_down.weight"], f32), sd["proj_down.bias"])
        idx = search(rD, books, rate.beam, books_use)[0].astype(np.int64)
        idx = idx.reshape(idx.shape[0], B, n)
        qD, v, c, _ = rt.rate_chunk(rD, books, idx, rate, packet_tok)
        z_run[..., s:e] = ro._proj_up(orc, sd, qD, residual=z_pred)
        ids.append(idx); nbv.append(v); nbs.append(c); rDs.append(rD)
    cat = lambda xs: np.concatenate(xs, axis=-1)
    return z_run, cat(ids), cat(nbv), cat(nbs), cat(rDs)
