"""CPU restatement of the audio transport (include/mvq.h: mvq_dac_rvq_from_codes_layers_f32, mvq_dac_rvq_rate_f32; DESIGN.md section
19), from numpy float32 operations (each one IEEE fp32 operation), orc.conv1d (the fma chain of out_proj) and the pieces of
tests/receiver_oracle.py, tests/rate_oracle.py and tests/lossy_oracle.py.  Shared by tests/test_av_cpu.py and tests/test_gpu_av.py.

The quantiser is three raw arrays: cb[nq, K, 8] (codebooks), ow[nq, C, 8] (out_proj weights, weight norm folded), ob[nq, C].

  * stages: zq_i = out_proj_i(cb_i[clip(code_i)]) per stage (receiver_oracle.from_codes's own step);
  * from_codes_layers: token (b, t) sums its first min(nq, count[b, t]) stages, ((0 + zq_0) + zq_1) + ...; count 0 is +0;
  * energies: d_m = z - S_m, p = d*d, E_m summed in the fixed order of include/mvq.h (4 strided channels, 16 groups, the slabs);
  * rate_audio: energies + rate_oracle.decide per item + from_codes_layers on the counts;
  * closed_loop_av: rate_audio, then rate_oracle.closed_loop_ar on that qa; receiver_av: the receiver fed counts on both streams.
"""
import numpy as np

import lossy_oracle as lo
import rate_oracle as rt

f32 = np.float32
K_AUDIO = 1024


def quantiser(seed, nq=32, K=K_AUDIO, C=1024):
    """Seeded raw quantiser tensors (cb, ow, ob)."""
    r = np.random.default_rng(seed)
    return ((r.standard_normal((nq, K, 8)) * 0.3).astype(f32), (r.standard_normal((nq, C, 8)) * 0.2).astype(f32),
            (r.standard_normal((nq, C)) * 0.02).astype(f32))


def quantiser_of(orc, sd, prefix="A_QUANT."):
    """The same three arrays from a model state dict."""
    cb, ow, ob = [], [], []
    while f"{prefix}quantizers.{len(cb)}.codebook.weight" in sd:
        p = f"{prefix}quantizers.{len(cb)}"
        w, b = orc._wn(sd, p + ".out_proj")
        cb.append(np.asarray(sd[p + ".codebook.weight"], f32)); ow.append(np.asarray(w, f32).reshape(w.shape[0], -1)); ob.append(np.asarray(b, f32))
    return np.stack(cb), np.stack(ow), np.stack(ob)


def stages(orc, cb, ow, ob, codes, nq=None):
    """codes[B, >= nq, T] -> [zq_0, ..., zq_{nq-1}], each [B, C, T]; codes clamped to [0, K)."""
    codes = np.asarray(codes, np.int64)
    nq = min(codes.shape[1], cb.shape[0]) if nq is None else int(nq)
    out = []
    for i in range(nq):
        z_p = np.ascontiguousarray(cb[i][np.clip(codes[:, i], 0, cb.shape[1] - 1)].transpose(0, 2, 1))   # raw rows [B, 8, T]
        out.append(orc.conv1d(z_p, np.ascontiguousarray(ow[i][:, :, None]), ob[i]))
    return out


def from_codes_layers(orc, cb, ow, ob, codes, count, nq=None, zs=None):
    """-> qa[B, C, T]: token (b, t) = ((0 + zq_0) + zq_1) + ... over its first min(nq, count[b, t]) stages."""
    zs = stages(orc, cb, ow, ob, codes, nq) if zs is None else zs
    B, _, T = np.asarray(codes).shape
    count = np.minimum(np.asarray(count).astype(np.int64), len(zs))
    S = np.zeros((B, ow.shape[1], T), f32)
    out = np.zeros_like(S)
    for m in range(len(zs) + 1):
        sel = count == m                                                 # [B, T]
        out = np.where(sel[:, None, :], S, out)
        if m < len(zs):
            S = S + zs[m]
    return out


def energy_sum(p):
    """p[B, C, T] -> [B, T]: the fixed order.  c = 64 s + 16 u + g: over u (4 terms) from +0, over g (16) from +0, over s from +0."""
    B, C, T = p.shape
    q = p.reshape(B, C // 64, 4, 16, T)
    t = np.zeros((B, C // 64, 16, T), f32)
    for u in range(4):
        t = t + q[:, :, u]
    P = np.zeros((B, C // 64, T), f32)
    for g in range(16):
        P = P + t[:, :, g]
    E = np.zeros((B, T), f32)
    for s in range(C // 64):
        E = E + P[:, s]
    return E


def energies(z, zs):
    """z[B, C, T] and the stage outputs -> E float32 [nq + 1, B, T]."""
    z = np.asarray(z, f32)
    S = np.zeros_like(z)
    E = []
    with np.errstate(invalid="ignore", over="ignore"):
        for m in range(len(zs) + 1):
            d = z - S
            E.append(energy_sum(d * d))
            if m < len(zs):
                S = S + zs[m]
    return np.stack(E)


def rate_audio(orc, cb, ow, ob, z, codes, rate, packet_tok, na_use=None):
    """-> (qa[B, C, T] the receiver's sum over each token's count, na_valid uint8 [B, T], na_sent uint8 [B, P], E[na + 1, B, T])."""
    zs = stages(orc, cb, ow, ob, codes, na_use)
    E = energies(z, zs)
    B, _, T = np.asarray(z).shape
    na_sent = np.stack([rt.decide(E[:, b], rate, packet_tok) for b in range(B)]).astype(np.uint8)
    na_valid = rt.expand(na_sent, T, packet_tok)
    return from_codes_layers(orc, cb, ow, ob, codes, na_valid, zs=zs), na_valid, na_sent, E


def layered_inputs(orc, cb, ow, ob, B, T, nq, seed, noise=1e-3):
    """Inputs on which the rule has something to decide: random codes (a few out of range) and
    z[:, :, t] = from_codes(codes[:, :m_t])[:, :, t] + small noise, m_t varied per token.  -> (z, codes, m_t)."""
    r = np.random.default_rng(seed)
    K = cb.shape[1]
    codes = r.integers(0, K, size=(B, nq, T))
    flat = codes.reshape(-1)
    flat[r.integers(0, flat.size, size=max(1, flat.size // 50))] = K + 5
    flat[r.integers(0, flat.size, size=max(1, flat.size // 50))] = -3
    m_t = r.integers(0, nq + 1, size=(B, T))
    z = from_codes_layers(orc, cb, ow, ob, codes, m_t, nq)
    z = (z + noise * r.standard_normal(z.shape)).astype(f32)
    return z, codes, m_t


def closed_loop_av(orc, sd, q3, za, codes, zt, rate, audio_rate, packet_tok=lo.PACKET_TOK, audio_books=None):
    """The whole-item sender with both loops closed -> (z_run, idx, nb_valid, nb_sent, na_valid, na_sent, qa)."""
    qa, na_valid, na_sent, _ = rate_audio(orc, *q3, za, codes, audio_rate, packet_tok, audio_books)
    z_run, idx, nb_valid, nb_sent, _ = rt.closed_loop_ar(orc, sd, qa, zt, rate, packet_tok)
    return z_run, idx, nb_valid, nb_sent, na_valid, na_sent, qa


def receiver_av(orc, sd, q3, codes, idx, nb_valid, na_valid, na_use=None):
    """The receiver fed counts on both streams: qa from the stages that arrived (a token with none: +0), then the lossy loop."""
    qa = from_codes_layers(orc, *q3, codes, na_valid, na_use)
    return lo.lossy_loop(orc, sd, qa, idx, nb_valid)
