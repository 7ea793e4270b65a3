"""Case tables of the three forward launchers that choose a kernel by token count, width and alignment (LayerNorm, the
RVQ-EMA search, the DAC residual VQ), shared by tests/test_forward_forms_host.py (dispatch, oracle against float64) and
tests/test_gpu_forward_forms.py (kernel against oracle).  Every case lists its shape, its options and the kernel it must
run, as ops.*_kernel_name reports it; inputs are seeded from the case tuple.  Shapes are the smallest that reach a form or
an edge of its code, not workload shapes."""
import functools
import math
import zlib

import numpy as np

_ORACLE = {}


def oracle_result(kind, case, orc):
    """The oracle's answer for a case, computed once per session and shared (read-only) by every test that needs it."""
    key = (kind, case)
    if key not in _ORACLE:
        if kind == "ln":
            i, (eps, do_tanh, post_scale) = ln_inputs(case), ln_params(case[3])
            out = (orc.layernorm_c(i["v"], i["gamma"], i["beta"], eps, do_tanh, post_scale),)
        elif kind == "rvq":
            z, books = rvq_inputs(case)
            out = orc.rvq_ema_forward(z, list(books), case[5])
        else:
            sd, z, _ = dac_inputs(case)
            out = orc.dac_quantizer(sd, z, case[3])[:3]
        for a in out:
            a.setflags(write=False)
        _ORACLE[key] = out
    return _ORACLE[key]


# ------------------------------------------------------------------------------------------------------------ LayerNorm
LN_LAT,LN_T8, LN_T4, LN_SCALAR = ("layernorm_c_lat_kernel", "layernorm_c_tile_kernel<8>", "layernorm_c_tile_kernel<4>",
                                   "layernorm_c_kernel")
LN_FORMS = (LN_LAT, LN_T8, LN_T4, LN_SCALAR)
# options: "pe" (positional table added), "sub" (x - sub), "tanh" (do_tanh with post_scale 0.08), "scale" (post_scale 0.37, no
# tanh), "eps6" (eps = 1e-6 instead of 1e-5), "folded" (the token-folded [1, C, B*T] layout)
LN_OPTIONS = (("pe",), ("sub",), ("sub", "pe"), ("tanh",), ("scale",), ("eps6",), ("folded",))
# (B, C, T, options, form)
LN_CASES = [
    # latency form: n <= 1024, C % 64 == 0 (C <= 1216).  C = 64: one pass with clamped channel indices; C = 1088 / 1216: a second,
    # partial pass that reloads gamma / beta; n = 5: tail of a 4-token task; n = 1024: the limit
    (1, 64, 1, (), LN_LAT),
    (1, 64, 5, ("pe",), LN_LAT),
    (3, 1024, 7, ("sub",), LN_LAT),
    (2, 1088, 5, ("sub", "pe"), LN_LAT),
    (1, 1216, 9, ("tanh",), LN_LAT),
    (4, 64, 256, ("scale",), LN_LAT),
    (2, 1024, 3, ("eps6",), LN_LAT),
    (5, 1088, 13, ("folded",), LN_LAT),
    (1, 1152, 5, (), LN_LAT),
    (8, 1024, 128, ("folded", "pe"), LN_LAT),
    # 8-token tiles: n > 64 and (n > 1024 or C % 64 != 0).  n = 1025: first count past the latency form, a last tile of one token;
    # C = 8: below one 16-channel batch; 24: one batch + scalar tail; 48: an odd number of batches; 72, 200: both; 1278: the widest
    (1, 1024, 1025, (), LN_T8),
    (5, 8, 13, ("pe",), LN_T8),
    (2, 24, 65, ("sub",), LN_T8),
    (1, 48, 65, ("sub", "pe"), LN_T8),
    (5, 72, 26, ("tanh",), LN_T8),
    (1, 200, 65, ("scale",), LN_T8),
    (13, 1278, 5, ("eps6",), LN_T8),
    (5, 200, 26, ("folded",), LN_T8),
    (2, 1278, 65, (), LN_T8),
    # 4-token tiles: n <= 64 and C % 64 != 0
    (1, 8, 1, (), LN_T4),
    (1, 72, 5, ("pe",), LN_T4),
    (4, 200, 16, ("sub",), LN_T4),
    (1, 8, 5, ("sub", "pe"), LN_T4),
    (2, 72, 32, ("tanh",), LN_T4),
    (1, 200, 1, ("scale",), LN_T4),
    (5, 200, 1, ("eps6",), LN_T4),
    (4, 8, 16, ("folded",), LN_T4),
    (1, 72, 1, (), LN_T4),
    # one thread per token: C > 1278 (1280: a multiple of 64 that is still too wide)
    (1, 1279, 5, (), LN_SCALAR),
    (2, 1280, 65, ("pe",), LN_SCALAR),
    (5, 1279, 1, ("sub",), LN_SCALAR),
    (1, 1280, 5, ("sub", "pe"), LN_SCALAR),
    (1, 1279, 130, ("tanh",), LN_SCALAR),
    (5, 1280, 1, ("scale",), LN_SCALAR),
    (1, 1280, 5, ("eps6",), LN_SCALAR),
    (5, 1279, 26, ("folded",), LN_SCALAR),
]


def _seed(*parts):
    return zlib.crc32(repr(parts).encode())


def ln_id(case):
    B, C, T, opts, _ = case
    return f"B{B}-C{C}-T{T}-" + ("+".join(opts) or "plain")


def ln_params(opts):
    """(eps, do_tanh, post_scale) of a case's options."""
    return (1e-6 if "eps6" in opts else 1e-5, "tanh" in opts, 0.08 if "tanh" in opts else (0.37 if "scale" in opts else 1.0))


@functools.lru_cache(maxsize=None)
def ln_inputs(case):
    """-> dict(x, sub, pe, gamma, beta, v): x[B,C,T] zero-mean, unit-variance like the model's activations; sub / pe are None
    unless the case asks for them; v = (x - sub) + pe formed in fp32, in that order -- what every kernel normalises."""
    B, C, T, opts, _ = case
    r = np.random.default_rng(_seed("ln", B, C, T, opts))
    x = r.standard_normal((B, C, T)).astype(np.float32)
    sub = (0.5 * r.standard_normal((B, C, T))).astype(np.float32) if "sub" in opts else None
    pe = r.uniform(-1.0, 1.0, (T, C)).astype(np.float32) if "pe" in opts else None
    gamma = r.uniform(0.5, 1.5, C).astype(np.float32)
    beta = (0.1 * r.standard_normal(C)).astype(np.float32)
    v = x
    if sub is not None:
        v = v - sub
    if pe is not None:
        v = v + pe.T[None]
    for a in (x, sub, pe, gamma, beta, v):
        if a is not None:
            a.setflags(write=False)
    return dict(x=x, sub=sub, pe=pe, gamma=gamma, beta=beta, v=v)


def ln_float64(v, gamma, beta, eps, do_tanh, post_scale):
    """nn.LayerNorm over the channel axis of v[B,C,T] (biased variance), then tanh and the scale, in float64."""
    v = v.astype(np.float64)
    mean = v.mean(axis=1, keepdims=True)
    var = ((v - mean) ** 2).mean(axis=1, keepdims=True)
    y = (v - mean) / np.sqrt(var + np.float64(np.float32(eps))) * gamma.astype(np.float64)[None, :, None] + beta.astype(np.float64)[None, :, None]
    if do_tanh:
        y = np.tanh(y)
    return np.float64(np.float32(post_scale)) * y


def fold(a):
    """[B, C, T] -> the token-folded [1, C, B*T] layout (item b's tokens at columns b*T .. b*T + T - 1)."""
    B, C, T = a.shape
    return np.ascontiguousarray(a.transpose(1, 0, 2).reshape(1, C, B * T))


def unfold(a, B):
    _, C, BT = a.shape
    return np.ascontiguousarray(a.reshape(C, B, BT // B).transpose(1, 0, 2))


# ----------------------------------------------------------------------------------------------------------- RVQ search
RVQ_ROWS, RVQ_TOKEN, RVQ_T8, RVQ_T32 = ("rvq_ema_forward_rows_kernel<24>", "rvq_ema_forward_token_kernel",
                                        "rvq_ema_forward_kernel<8>", "rvq_ema_forward_kernel<32>")
RVQ_MFMA16, RVQ_MFMA32 = "rvq_ema_forward_mfma_kernel [tpb=16]", "rvq_ema_forward_mfma_kernel [tpb=32]"
RVQ_FORMS = (RVQ_ROWS, RVQ_TOKEN, RVQ_T8, RVQ_MFMA16, RVQ_MFMA32, RVQ_T32)
TIE_CODES = (17, 40, 300, 499)      # exact duplicates of one code; every token is that code, so every index must be 17
# (B, D, T, nb, K, use, tie, form)
RVQ_CASES = [
    # rows: N <= 256, D == 96, K <= 512, aligned books.  K = 500: the last wave of codes is partial
    (1, 96, 1, 2, 500, None, False, RVQ_ROWS),
    (4, 96, 64, 2, 512, 1, False, RVQ_ROWS),
    (2, 96, 5, 3, 500, None, False, RVQ_ROWS),
    (1, 96, 5, 1, 512, None, True, RVQ_ROWS),
    # token: N <= 256 otherwise.  D = 20: the `d + 4u < D` guard of the 16-wide row walk; K = 3: most threads own no code
    (2, 64, 5, 2, 512, None, False, RVQ_TOKEN),
    (1, 96, 7, 2, 1024, None, False, RVQ_TOKEN),
    (3, 128, 5, 2, 300, 1, False, RVQ_TOKEN),
    (1, 20, 9, 2, 100, None, False, RVQ_TOKEN),
    (1, 4, 3, 2, 3, None, False, RVQ_TOKEN),
    (4, 64, 64, 1, 512, None, False, RVQ_TOKEN),
    (1, 96, 5, 1, 1024, None, True, RVQ_TOKEN),
    # 8-token tiles: 256 < N < 1024, or N < 4096 where the MFMA form is not eligible.  K = 500: a second LDS pass of 244 codes;
    # K = 301: one of 45, which is no multiple of 4 -> the row-major staging order; N % 8 != 0 everywhere but 1024
    (1, 96, 257, 2, 512, None, False, RVQ_T8),
    (3, 96, 341, 1, 128, None, False, RVQ_T8),
    (2, 96, 515, 2, 500, 1, False, RVQ_T8),
    (1, 96, 1030, 1, 301, None, False, RVQ_T8),
    (1, 20, 259, 2, 100, None, False, RVQ_T8),
    (1, 64, 300, 1, 512, None, False, RVQ_T8),
    (1, 128, 261, 1, 300, None, False, RVQ_T8),
    (1, 96, 300, 1, 512, None, True, RVQ_T8),
    # D = 128 with many tokens: neither the MFMA form (167 168 bytes of LDS) nor the 32-token tile (165 632) fits 160 KiB
    (1, 128, 4097, 1, 256, None, False, RVQ_T8),
    # MFMA, 16 live tokens per block: 1024 <= N < 8161, K % 32 == 0.  (D 64, K 1024): four LDS passes; (D 4, K 32): one MFMA k-step pair
    (1, 96, 1024, 2, 512, None, False, RVQ_MFMA16),
    (2, 96, 515, 2, 512, 1, False, RVQ_MFMA16),
    (1, 64, 1030, 1, 1024, None, False, RVQ_MFMA16),
    (1, 4, 1030, 2, 32, None, False, RVQ_MFMA16),
    (1, 96, 1100, 1, 512, None, True, RVQ_MFMA16),
    # MFMA, 32 live tokens per block: N >= 8161.  N = 8175: a last block of 15
    (109, 96, 75, 2, 512, None, False, RVQ_MFMA32),
    (1, 96, 8161, 2, 512, 1, True, RVQ_MFMA32),
    # 32-token tiles: N >= 4096 where the MFMA form is not eligible (K % 32 != 0)
    (1, 32, 4097, 2, 100, None, False, RVQ_T32),
    (1, 32, 4097, 2, 100, 1, False, RVQ_T32),
    (1, 96, 4096, 1, 500, None, True, RVQ_T32),
]


# Mixed into every seed.  A float64 arg-max can vouch for an fp32 one only where the best two scores are clearly apart
# (RVQ_MIN_GAP, two orders above fp32 round-off of scores of order 1); among the 16 350 searches of the largest case a draw
# usually holds one or two closer pairs, so the salt is the first (counting from 0) for which NO search of the table comes
# nearer than 1.5e-5: the smallest gap of the table is then 1.88e-5, and the share of tokens the host test leaves out is 0,
# which it asserts.
RVQ_SALT = 26
RVQ_MIN_GAP = 1e-5


def rvq_id(case):
    B, D, T, nb, K, use, tie, _ = case
    return f"B{B}-D{D}-T{T}-nb{nb}-K{K}-use{use}" + ("-tie" if tie else "")


@functools.lru_cache(maxsize=None)
def rvq_inputs(case):
    """-> (z[B,D,T], books[nb,K,D]).  Plain cases: unit-variance tokens, book i of scale 0.6^i / sqrt(D).  Tie cases: codes
    TIE_CODES of book 0 are one and the same row and every token IS that row."""
    B, D, T, nb, K, use, tie, _ = case
    r = np.random.default_rng(_seed("rvq", RVQ_SALT, B, D, T, nb, K, use, tie))
    books = np.stack([((0.6 ** i) * r.standard_normal((K, D)) / math.sqrt(D)).astype(np.float32) for i in range(nb)])
    if tie:
        for k in TIE_CODES[1:]:
            books[0, k] = books[0, TIE_CODES[0]]
        z = np.ascontiguousarray(np.broadcast_to(books[0, TIE_CODES[0]][None, :, None], (B, D, T))).astype(np.float32)
    else:
        z = r.standard_normal((B, D, T)).astype(np.float32)
    z.setflags(write=False); books.setflags(write=False)
    return z, books


def rvq_float64(z, books, use):
    """The residual search in float64: per stage, arg-max of r.e - |e|^2 / 2 (lowest index first), r -= e.
    -> (idx[nb_use, N], gap[nb_use, N]: best score minus second best)."""
    B, D, T = z.shape
    nb = books.shape[0] if use is None else min(use, books.shape[0])
    res = z.astype(np.float64).transpose(0, 2, 1).reshape(B * T, D).copy()
    idx = np.zeros((nb, B * T), np.int64)
    gap = np.zeros((nb, B * T))
    for i in range(nb):
        e = books[i].astype(np.float64)
        sc = res @ e.T - 0.5 * (e * e).sum(axis=1)[None]
        idx[i] = sc.argmax(axis=1)
        top = np.partition(sc, -2, axis=1)[:, -2:] if sc.shape[1] > 1 else np.stack([sc[:, 0] - np.inf, sc[:, 0]], axis=1)
        gap[i] = top[:, 1] - top[:, 0]
        res -= e[idx[i]]
    return idx, gap


# -------------------------------------------------------------------------------------------------------------- DAC RVQ
def dac_form(kind, C):
    return {"lat1": f"dac_rvq_lat_kernel<{C // 16}, 4, 1>", "lat2": f"dac_rvq_lat_kernel<{C // 16}, 4, 2>",
            "tile": f"dac_rvq_kernel<{C // 16}, 8>"}[kind]


DAC_KINDS = ("lat1", "lat2", "tile")
# (B, C, T, nq, K, prepared, nq_item, kind)
DAC_CASES = [
    # one token per block: N <= 256, K == 1024, prepared codebook
    (1, 256, 1, 2, 1024, True, None, "lat1"),
    (1, 512, 1, 3, 1024, True, None, "lat1"),
    (4, 1024, 64, 2, 1024, True, None, "lat1"),
    (1, 1024, 1, 32, 1024, True, None, "lat1"),
    (3, 512, 5, 3, 1024, True, (3, 1, 2), "lat1"),
    (2, 256, 128, 2, 1024, True, None, "lat1"),
    # two tokens per block: 256 < N <= 1024.  N = 297: the last block has one live token
    (3, 1024, 99, 2, 1024, True, None, "lat2"),
    (4, 256, 256, 2, 1024, True, None, "lat2"),
    (3, 512, 99, 3, 1024, True, (1, 3, 2), "lat2"),
    (1, 256, 257, 2, 1024, True, None, "lat2"),
    # 16-token tiles: everything else.  N = 1025: a last tile of one token; K = 256 with a prepared codebook; no prepared codebook
    (1, 1024, 1025, 2, 1024, True, None, "tile"),
    (1, 1024, 37, 3, 1024, False, None, "tile"),
    (2, 1024, 19, 2, 256, True, None, "tile"),
    (1, 256, 1025, 2, 1024, True, None, "tile"),
    (3, 512, 13, 3, 1024, False, (2, 3, 1), "tile"),
]


def dac_id(case):
    B, C, T, nq, K, prepared, nq_item, kind = case
    return f"B{B}-C{C}-T{T}-nq{nq}-K{K}-" + ("prep" if prepared else "raw") + ("-items" if nq_item else "")


@functools.lru_cache(maxsize=None)
def dac_inputs(case):
    """-> (sd, z, weights): sd = synth.quantizer_state of the case's width as numpy, z[B,C,T], weights = dict(in_w[nq,8,C],
    in_b, cb[nq,K,8], out_w[nq,C,8], out_b) with the weight norm folded by the oracle (what the modules hand to ops.dac_rvq)."""
    from multimodal_vqvae_compression_audio_tactile_amd import synth
    from oracle import oracle as orc
    B, C, T, nq, K, prepared, nq_item, kind = case
    seed = _seed("dac", B, C, T, nq, K, prepared, nq_item)
    sd = {k: v.numpy() for k, v in synth.quantizer_state(seed % 100000, n_codebooks=nq, K=K, c=C).items()}
    z = np.random.default_rng(seed).standard_normal((B, C, T)).astype(np.float32)
    wn = lambda p: orc.weight_norm(sd[p + ".weight_v"], sd[p + ".weight_g"])
    w = dict(in_w=np.stack([wn(f"quantizers.{i}.in_proj").reshape(8, C) for i in range(nq)]),
             out_w=np.stack([wn(f"quantizers.{i}.out_proj").reshape(C, 8) for i in range(nq)]),
             in_b=np.stack([sd[f"quantizers.{i}.in_proj.bias"] for i in range(nq)]),
             out_b=np.stack([sd[f"quantizers.{i}.out_proj.bias"] for i in range(nq)]),
             cb=np.stack([sd[f"quantizers.{i}.codebook.weight"] for i in range(nq)]))
    return sd, z, w
