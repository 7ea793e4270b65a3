"""CPU restatement of the streaming sender, from existing oracle pieces only (oracle.dac_encoder, oracle.cross_predictor and the
per-chunk body of oracle.proposed_encode_latents).  Shared by tests/test_sender_cpu.py and tests/test_gpu_sender.py.

  * split_pushes: the push patterns the tests feed a session (all pushes of m tokens, or seeded mixed 1..16);
  * scheduled_encode: the encoder over the windows of stream.sender_schedule, the exact tokens of each window concatenated;
  * ar_chunk / chunked_ar: the sender's quantisation loop run ONE chunk per call, the only thing carried between calls being
    z_prev = z_run[..., -1] of the chunk before.
"""
import numpy as np

from multimodal_vqvae_compression_audio_tactile_amd import stream

HOP = stream.HOP
CHUNK = stream.CHUNK_TOK


def enc_weights(seed=7):
    """The encoder weights of synth.dac_state(seed) as numpy, keys as oracle.dac_encoder(prefix="encoder.") reads them."""
    from multimodal_vqvae_compression_audio_tactile_amd import synth
    return {k: v.numpy() for k, v in synth.dac_state(seed=seed).items() if k.startswith("encoder.")}


def signal(L, B=1, seed=5):
    return (0.3 * np.random.default_rng(seed).standard_normal((B, 1, L))).astype(np.float32)


def split_pushes(L, pattern, seed=0):
    """Push sizes in tokens for an item of L samples: as many pushes of the pattern as fit, the rest is the tail of finish.
    pattern: an int m (all pushes of m tokens) or "mixed" (seeded, 1..16)."""
    whole = L // HOP
    out, used = [], 0
    r = np.random.default_rng(seed)
    while True:
        m = int(r.integers(1, stream.PUSH_MAX_TOK + 1)) if pattern == "mixed" else int(pattern)
        if used + m > whole:
            return out
        out.append(m)
        used += m


def scheduled_encode(orc, sd, x, pushes, halo=stream.ENC_HALO_TOK, prefix="encoder."):
    """Concatenation over stream.sender_schedule of the emitted tokens of each window's encode.  x[B, 1, L]."""
    L = x.shape[-1]
    T = stream.enc_tokens(L)
    out = []
    steps = stream.sender_schedule(T, pushes, halo=halo)
    for i, (w0, w1, c0, c1, _) in enumerate(steps):
        if c1 <= c0:
            continue
        last = i == len(steps) - 1                                     # finish: the window runs to the item's true end
        z = orc.dac_encoder(sd, np.ascontiguousarray(x[..., HOP * w0:(L if last else HOP * w1)]), prefix=prefix)
        assert z.shape[-1] == w1 - w0, (z.shape, w0, w1)
        out.append(z[..., CHUNK * c0 - w0:min(CHUNK * c1, T) - w0])
    return np.concatenate(out, axis=-1)


def _books(sd):
    books = []
    while f"vq.books.{len(books)}" in sd:
        books.append(np.asarray(sd[f"vq.books.{len(books)}"], np.float32))
    return books


def ar_chunk(orc, sd, qa_c, zt_c, z_prev, pe, books_use=None):
    """One chunk (<= 16 tokens) of oracle.proposed_encode_latents' loop: zt_prev is zero but for column 0 = z_prev (None: the
    first chunk) -> (z_hat [B, C, n], idx [nb, B, n])."""
    B, C, n = zt_c.shape
    assert n <= CHUNK
    zt_prev = np.zeros((B, C, n), np.float32)
    if z_prev is not None:
        zt_prev[..., 0] = z_prev
    scale = np.float32(min(max(float(np.float32(sd["scale"])), 5e-3), 0.5))
    z_pred = orc.cross_predictor(sd, zt_prev, qa_c, pe)
    rN = orc.layernorm_c(zt_c - z_pred, sd["tokennorm.ln.weight"], sd["tokennorm.ln.bias"], do_tanh=True, post_scale=scale)
    rD = orc.conv1d(rN, np.asarray(sd["proj_down.weight"], np.float32), sd["proj_down.bias"])
    qD, idx = orc.rvq_ema_forward(rD, _books(sd), books_use)
    z_hat = orc.conv1d(qD, np.asarray(sd["proj_up.weight"], np.float32), sd["proj_up.bias"], residual=z_pred)
    return z_hat, idx.reshape(idx.shape[0], B, n)


def chunked_ar(orc, sd, qa, zt, books_use=None):
    """The sequence one chunk per call, z_prev carried -> (z_run, idx)."""
    C, Tlat = zt.shape[1], zt.shape[2]
    pe = np.asarray(sd["predict.pos.pe"], np.float32) if "predict.pos.pe" in sd else orc.pos_table(C)
    zs, ids, z_prev = [], [], None
    for s in range(0, Tlat, CHUNK):
        e = min(Tlat, s + CHUNK)
        z, idx = ar_chunk(orc, sd, np.ascontiguousarray(qa[..., s:e]), np.ascontiguousarray(zt[..., s:e]), z_prev, pe, books_use)
        z_prev = z[..., -1].copy()
        zs.append(z)
        ids.append(idx)
    return np.concatenate(zs, axis=-1), np.concatenate(ids, axis=-1)
