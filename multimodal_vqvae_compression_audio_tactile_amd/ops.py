"""Tensor-level wrappers over the C ABI (include/mvq.h).

torch is plumbing here: device memory (caching allocator), the current HIP stream and nothing else.
Every op takes fp32 tensors on a HIP device, launches on ``torch.cuda.current_stream()`` and returns
freshly allocated outputs.  Inputs arriving in another dtype (e.g. fp16 under the reference's CUDA AMP
autocast, Evaluation/compare_dacvsproposal_5_eval.py:441) are widened to fp32: the path computes in fp32.
"""
from __future__ import annotations

import ctypes
import operator

import torch

from . import _lib
from ._lib import MvqError, check
from .stream import resample_stream_out_len, resample_stream_rational_out_len  # noqa: F401  (host arithmetic, kept where no torch is needed)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(t: torch.Tensor, name: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor")
    if t.device.type != "cuda":
        raise MvqError(f"{name}: tensor is on {t.device}; the MI355X path has no CPU fallback")
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


def _p(t):
    return None if t is None else t.data_ptr()


def conv1d_out_len(tin, ks, stride=1, dil=1, pad=0):
    span = tin + 2 * pad - dil * (ks - 1) - 1
    return 0 if span < 0 else span // stride + 1


def conv_kernel_name(cin, cout, ks, stride=1, dil=1, transposed=False, tin=24000, batch=64) -> str:
    """Kernel instantiation the library launches for this conv shape (as rocprofv3 names it)."""
    import ctypes
    buf = ctypes.create_string_buffer(160)
    check(_lib.lib().mvq_conv_kernel_name(batch, cin, cout, ks, stride, dil, int(transposed), tin, buf, 160),
          "mvq_conv_kernel_name")
    return buf.value.decode()


def _kernel_name(entry: str, *args) -> str:
    buf = ctypes.create_string_buffer(160)
    check(getattr(_lib.lib(), entry)(*args, buf, 160), entry)
    return buf.value.decode()


def layernorm_kernel_name(batch, c, t) -> str:
    """Kernel instantiation ops.layernorm_c launches for batch * t tokens of c channels (host arithmetic, no device)."""
    return _kernel_name("mvq_layernorm_kernel_name", int(batch), int(c), int(t))


def rvq_ema_forward_kernel_name(batch, dim, t, k, books_aligned=True) -> str:
    """Kernel instantiation ops.rvq_ema_forward (and the assignment pass of rvq_ema_step_) launches; the MFMA form's name ends
    in its live tokens per block, ``[tpb=16]`` or ``[tpb=32]``.  ``books_aligned``: the books tensor is 16-byte aligned."""
    return _kernel_name("mvq_rvq_ema_forward_kernel_name", int(batch), int(dim), int(t), int(k), int(bool(books_aligned)))


def dac_rvq_kernel_name(batch, c, t, k, prepared=True, aligned=True) -> str:
    """Kernel instantiation ops.dac_rvq launches.  ``prepared``: dac_rvq_prepare's tensors are passed; ``aligned``: in_w, out_w,
    the codebook and the prepared codebook are all 16-byte aligned."""
    return _kernel_name("mvq_dac_rvq_kernel_name", int(batch), int(c), int(t), int(k), int(bool(prepared)), int(bool(aligned)))


def weight_norm(v: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    """w = v * (g / ||v||) over dim 0 rows (old-style torch weight_norm fold)."""
    v = _dev(v, "v"); g = _dev(g, "g")
    w = torch.empty_like(v)
    rows = v.shape[0]
    check(_lib.lib().mvq_weight_norm_f32(v.data_ptr(), g.data_ptr(), w.data_ptr(), rows, v.numel() // rows, _stream()),
          "mvq_weight_norm_f32")
    return w


def pack_conv1d(w: torch.Tensor) -> torch.Tensor:
    """torch layout w[Cout, Cin, ks] -> K-major packed image used by conv1d()."""
    w = _dev(w, "w")
    cout, cin, ks = w.shape
    n = _lib.lib().mvq_conv1d_packed_floats(cin, cout, ks)
    wp = torch.empty(n, device=w.device, dtype=torch.float32)
    check(_lib.lib().mvq_conv1d_pack_f32(w.data_ptr(), wp.data_ptr(), cin, cout, ks, _stream()), "mvq_conv1d_pack_f32")
    return wp


def pack_conv_transpose1d(w: torch.Tensor, stride: int) -> torch.Tensor:
    """torch layout w[Cin, Cout, 2*stride] -> polyphase packed image used by conv_transpose1d()."""
    w = _dev(w, "w")
    cin, cout, ks = w.shape
    if ks != 2 * stride:
        raise MvqError(f"conv_transpose1d: kernel {ks} != 2*stride ({stride}) is outside the path")
    n = _lib.lib().mvq_conv_transpose1d_packed_floats(cin, cout, stride)
    wp = torch.empty(n, device=w.device, dtype=torch.float32)
    check(_lib.lib().mvq_conv_transpose1d_pack_f32(w.data_ptr(), wp.data_ptr(), cin, cout, stride, _stream()),
          "mvq_conv_transpose1d_pack_f32")
    return wp


def conv1d(x, wp, cout, ks, bias=None, stride=1, dil=1, pad=0, alpha_in=None, residual=None, alpha_out=None,
           tanh=False, out=None, alpha_dual=None, tvalid=0, gelu=False):
    """alpha_dual: also return snake(y_raw, alpha_dual) (the next ResidualUnit's Snake, hoisted): -> (y, y2).
    tvalid: rows are zero-padded beyond column tvalid (see include/mvq.h "Zero-padded rows"); 0 = plain tensors."""
    x = _dev(x, "x")
    B, cin, tin = x.shape
    tout = conv1d_out_len(tin, ks, stride, dil, pad)
    if out is None:
        out = torch.empty(B, cout, tout, device=x.device, dtype=torch.float32)
    y2 = torch.empty_like(out) if alpha_dual is not None else None
    if residual is not None:
        residual = _dev(residual, "residual")
        if tuple(residual.shape) != (B, cout, tout):
            raise MvqError(f"conv1d: residual shape {tuple(residual.shape)} != {(B, cout, tout)}")
    check(_lib.lib().mvq_conv1d_padded_f32(x.data_ptr(), wp.data_ptr(), _p(bias), _p(alpha_in), _p(residual),
                                           _p(alpha_out), out.data_ptr(), _p(y2), _p(alpha_dual), B, cin, tin, cout, ks,
                                           stride, dil, pad, 1 if tanh else (2 if gelu else 0), int(tvalid), _stream()), "mvq_conv1d_f32")
    return out if alpha_dual is None else (out, y2)


def build_flags() -> int:
    """mvq_build_flags() (include/mvq.h): 0 = no A/B override in the environment."""
    return _lib.build_flags()


def profile_begin() -> None:
    """Start bracketing every conv / residual-unit kernel launch with HIP events on its launch stream (include/mvq.h)."""
    check(_lib.lib().mvq_profile_begin(), "mvq_profile_begin")


def profile_reserve(n_launches: int) -> None:
    """Pre-create the event pairs of `n_launches` kernel launches (keeps hipEventCreate out of a timed region)."""
    check(_lib.lib().mvq_profile_reserve(int(n_launches)), "mvq_profile_reserve")


def profile_end() -> dict:
    """Stop and collect: {kernel instantiation name: {"seconds", "flops", "launches"}} (synchronises)."""
    import ctypes
    cap = 1024
    buf = (_lib.ProfileEntry * cap)()
    n, total = ctypes.c_int(0), ctypes.c_int(0)
    check(_lib.lib().mvq_profile_end2(buf, cap, ctypes.byref(n), ctypes.byref(total)), "mvq_profile_end2")
    if total.value > n.value:        # never hand a truncated table to the roofline arithmetic
        raise MvqError(f"mvq_profile_end2: {total.value} kernel instantiations recorded, buffer holds {cap}")
    return {buf[i].kernel.decode(): {"seconds": buf[i].seconds, "flops": buf[i].flops, "launches": buf[i].launches}
            for i in range(n.value)}


def residual_unit_kernel_name(c, dil) -> str:
    import ctypes
    buf = ctypes.create_string_buffer(160)
    check(_lib.lib().mvq_residual_unit_kernel_name(c, dil, buf, 160), "mvq_residual_unit_kernel_name")
    return buf.value.decode()


def residual_unit_fused(x, w7p, b7, alpha_a, alpha_b, w1p, b1, dil, alpha_next=None, alpha_dual=None, tvalid=0, x_snaked=None):
    """The single-launch form (C in {64, 96, 128}).  x_snaked = snake_a(x) (the producer's dual output): staged as is."""
    B, C, T = x.shape
    y = torch.empty_like(x)
    y2 = torch.empty_like(x) if alpha_dual is not None else None
    if x_snaked is not None and x_snaked.shape != x.shape:
        raise MvqError("residual_unit: x_snaked must have the shape of x")
    check(_lib.lib().mvq_residual_unit_padded_f32(x.data_ptr(), _p(x_snaked), w7p.data_ptr(), _p(b7), alpha_a.data_ptr(),
                                                  alpha_b.data_ptr(), w1p.data_ptr(), _p(b1), _p(alpha_next), y.data_ptr(),
                                                  _p(y2), _p(alpha_dual), None, B, C, T, dil, int(tvalid), _stream()),
          "mvq_residual_unit_f32")
    return y if alpha_dual is None else (y, y2)


def residual_unit(x, w7p, b7, alpha_a, alpha_b, w1p, b1, dil, alpha_next=None, x_snaked=None, alpha_dual=None, tvalid=0, w7q=None):
    """x + conv1(snake(conv7_dil(snake(x)))) (+ the next Snake1d): one fused launch for C in {64,96,128}, else the
    two conv launches (Snake on load / on store in the first, skip + next Snake in the second's epilogue).
    x_snaked: snake_a(x) already produced by the previous layer's dual output (skips the staging-time Snake);
    alpha_dual: also return snake(y_raw, alpha_dual) for the next unit -> (y, y2).
    w7q: the layer's packed_mode() image of the 7-tap weights -- given only in an opt-in arithmetic mode (set_arith) for a unit the
    mode claims; None (the default) keeps every launch the exact kernel."""
    x = _dev(x, "x")
    B, C, T = x.shape
    # the fused single-launch form, unless an opt-in arithmetic mode claims the unit's 7-tap conv (then: split + matrix-core conv +
    # the exact 1x1 with its skip, as for the wide units)
    unfuse = w7q is not None and x_snaked is not None
    if _lib.lib().mvq_residual_unit_scratch_floats(B, C, T, dil) == 0 and not unfuse:
        return residual_unit_fused(x, w7p, b7, alpha_a, alpha_b, w1p, b1, dil, alpha_next, alpha_dual, tvalid, x_snaked)
    if x_snaked is not None and w7q is not None:      # opt-in modes (set_arith): non-parity, fp32-class
        h = conv1d_k7_mode(x_snaked, w7q, C, dil, bias=b7, alpha_out=alpha_b, tvalid=tvalid)
    elif x_snaked is not None:
        h = conv1d(x_snaked, w7p, C, 7, bias=b7, dil=dil, pad=3 * dil, alpha_out=alpha_b, tvalid=tvalid)
    else:
        h = conv1d(x, w7p, C, 7, bias=b7, dil=dil, pad=3 * dil, alpha_in=alpha_a, alpha_out=alpha_b, tvalid=tvalid)
    return conv1d(h, w1p, C, 1, bias=b1, residual=x, alpha_out=alpha_next, alpha_dual=alpha_dual, tvalid=tvalid)


# ---- opt-in, NON-PARITY arithmetic mode "bf16x6" (include/mvq.h; csrc/conv_k7_bf16.hip) ------------------------------------------
# The default ("f32") computes every conv as the exact fp32 fma chain of the arithmetic contract.  set_arith("bf16x6") routes the
# 7-tap convs of the wide ResidualUnits (C a multiple of 128, or of 96: C = 192) through the three-piece bf16 split: fp32-accurate,
# not bit-identical; everything else keeps the exact path.
_ARITH = "f32"


def set_arith(mode: str) -> None:
    global _ARITH
    if mode not in ("f32", "bf16x6", "f16x3"):
        raise MvqError(f"set_arith: unknown mode {mode!r} (f32 | bf16x6 | f16x3)")
    _ARITH = mode


def get_arith() -> str:
    return _ARITH


class arith:
    """``with ops.arith("f16x3"): ...`` -- an opt-in arithmetic mode for the duration of a block (restored on exit, also on an
    exception).  The mode is process-global state read at LAUNCH time: a hipGraph captured under one mode keeps it when replayed."""

    def __init__(self, mode: str):
        self.mode, self.prev = mode, None

    def __enter__(self):
        self.prev = get_arith()
        set_arith(self.mode)
        return self

    def __exit__(self, *exc):
        set_arith(self.prev)
        return False


def bf16x6_eligible(c: int) -> bool:
    if _ARITH not in ("bf16x6", "f16x3") or c % 16 != 0:
        return False
    return c % 128 == 0 or c % 96 == 0


def bf16x3_split(x):
    """x[B, C, T] fp32 -> the three-piece bf16 image [B][C/8][3][T][8] (a flat int16 tensor)."""
    x = _dev(x, "x")
    B, C, T = x.shape
    xs = torch.empty(B * C * T * 3, device=x.device, dtype=torch.int16)
    check(_lib.lib().mvq_bf16x3_split_f32(x.data_ptr(), xs.data_ptr(), B, C, T, _stream()), "mvq_bf16x3_split_f32")
    return xs


def pack_conv1d_k7_bf16x3(w, dgrad=False):
    """Folded weights w[Cout, Cin, 7] fp32 -> the packed three-piece bf16 image of mvq_conv1d_k7_bf16x6_f32.
    dgrad: the input-gradient image instead (rows = Cin, k-channels = Cout, taps reversed)."""
    w = _dev(w, "w").contiguous()
    cout, cin, ks = w.shape
    if dgrad:
        cout, cin = cin, cout
    n = _lib.lib().mvq_conv1d_k7_bf16x3_packed_bytes(cout, cin)
    if ks != 7 or n == 0:
        raise MvqError(f"pack_conv1d_k7_bf16x3: needs [Cout % 128 == 0 or % 96 == 0, Cin % 16 == 0, 7], got {tuple(w.shape)}")
    wq = torch.empty(n // 2, device=w.device, dtype=torch.int16)
    check(_lib.lib().mvq_conv1d_k7_pack_bf16x3(w.data_ptr(), wq.data_ptr(), cout, cin, 1 if dgrad else 0, _stream()), "mvq_conv1d_k7_pack_bf16x3")
    return wq


def conv1d_k7_bf16x6(xs, wq, batch, cin, t, cout, dil, bias=None, alpha_out=None, tvalid=0, dual=False, dsn_src=None, dsn_alpha=None,
                     residual=None):
    """y[B, cout, t] = snake_out(conv7_dil(xs) + bias) on the bf16x6 matrix path; xs from bf16x3_split, wq from pack_conv1d_k7_bf16x3.
    dual: -> (conv + bias, snake_out of it).  dsn_src / dsn_alpha / residual: the input-gradient epilogue (wq packed with dgrad=True)."""
    y = torch.empty(batch, cout, t, device=xs.device, dtype=torch.float32)
    y2 = torch.empty_like(y) if dual else None
    check(_lib.lib().mvq_conv1d_k7_bf16x6_f32(xs.data_ptr(), wq.data_ptr(), _p(bias), _p(alpha_out), y.data_ptr(), _p(y2), _p(dsn_src),
                                              _p(dsn_alpha), _p(residual), batch, cin, t, cout, dil, int(tvalid), _stream()),
          "mvq_conv1d_k7_bf16x6_f32")
    return (y, y2) if dual else y


def f16x2_split(x):
    """x[B, C, T] fp32 -> (two-piece fp16 image [B][C/8][2][T][8] as a flat int16 tensor, per-item |x| maxima as int32 bit patterns)."""
    x = _dev(x, "x")
    B, C, T = x.shape
    xs = torch.empty(B * C * T * 2, device=x.device, dtype=torch.int16)
    xamax = torch.empty(max(B, 1), device=x.device, dtype=torch.int32)
    check(_lib.lib().mvq_f16x2_split_f32(x.data_ptr(), xs.data_ptr(), xamax.data_ptr(), B, C, T, _stream()), "mvq_f16x2_split_f32")
    return xs, xamax


def pack_conv1d_k7_f16x2(w, dgrad=False):
    """Folded weights w[Cout, Cin, 7] fp32 -> (packed two-piece fp16 image, the tensor's |w| maximum as an int32 bit pattern).
    dgrad: the input-gradient image instead (rows = Cin, k-channels = Cout, taps reversed)."""
    w = _dev(w, "w").contiguous()
    cout, cin, ks = w.shape
    if dgrad:
        cout, cin = cin, cout
    n = _lib.lib().mvq_conv1d_k7_f16x2_packed_bytes(cout, cin)
    if ks != 7 or n == 0:
        raise MvqError(f"pack_conv1d_k7_f16x2: needs [Cout % 128 == 0 or % 96 == 0, Cin % 16 == 0, 7], got {tuple(w.shape)}")
    wq = torch.empty(n // 2, device=w.device, dtype=torch.int16)
    wamax = torch.empty(1, device=w.device, dtype=torch.int32)
    check(_lib.lib().mvq_conv1d_k7_pack_f16x2(w.data_ptr(), wq.data_ptr(), wamax.data_ptr(), cout, cin, 1 if dgrad else 0, _stream()),
          "mvq_conv1d_k7_pack_f16x2")
    return wq, wamax


def conv1d_k7_f16x3(xs, xamax, wq, wamax, batch, cin, t, cout, dil, bias=None, alpha_out=None, tvalid=0, dual=False, dsn_src=None,
                    dsn_alpha=None, residual=None):
    """y[B, cout, t] = snake_out(conv7_dil(xs) + bias) with two fp16 pieces per operand (three piece products); dual / dsn_* /
    residual as in conv1d_k7_bf16x6."""
    y = torch.empty(batch, cout, t, device=xs.device, dtype=torch.float32)
    y2 = torch.empty_like(y) if dual else None
    check(_lib.lib().mvq_conv1d_k7_f16x3_f32(xs.data_ptr(), xamax.data_ptr(), wq.data_ptr(), wamax.data_ptr(), _p(bias), _p(alpha_out),
                                             y.data_ptr(), _p(y2), _p(dsn_src), _p(dsn_alpha), _p(residual), batch, cin, t, cout, dil,
                                             int(tvalid), _stream()), "mvq_conv1d_k7_f16x3_f32")
    return (y, y2) if dual else y


def conv1d_k7_mode(x, wq, cout, dil, bias=None, alpha_out=None, tvalid=0, dual=False, dsn_src=None, dsn_alpha=None, residual=None):
    """The current opt-in mode's 7-tap conv on an fp32 input x[B, C, T]: split pass + matrix-core conv.  wq: what the layer's
    packed_mode() / packed_mode_dgrad() returned for this mode."""
    x = _dev(x, "x")
    B, C, T = x.shape
    kw = dict(bias=bias, alpha_out=alpha_out, tvalid=tvalid, dual=dual, dsn_src=dsn_src, dsn_alpha=dsn_alpha, residual=residual)
    if _ARITH == "f16x3":
        xs, xamax = f16x2_split(x)
        return conv1d_k7_f16x3(xs, xamax, wq[0], wq[1], B, C, T, cout, dil, **kw)
    if _ARITH == "bf16x6":
        return conv1d_k7_bf16x6(bf16x3_split(x), wq, B, C, T, cout, dil, **kw)
    raise MvqError("conv1d_k7_mode: no opt-in arithmetic mode is set")


def conv_transpose1d(x, wp, cout, stride, pad, bias=None, alpha_in=None, alpha_out=None, alpha_dual=None, tout_rows=0,
                     tvalid=0, output_padding=0):
    """tout_rows / tvalid: zero-padded rows (include/mvq.h): row length of the output and its true length.
    output_padding: torch's ConvTranspose1d argument (that many more samples at the end of each row)."""
    x = _dev(x, "x")
    B, cin, tin = x.shape
    tout = int(tout_rows) if tout_rows else (tin - 1) * stride - 2 * pad + 2 * stride + int(output_padding)
    out = torch.empty(B, cout, max(tout, 0), device=x.device, dtype=torch.float32)
    y2 = torch.empty_like(out) if alpha_dual is not None else None
    check(_lib.lib().mvq_conv_transpose1d_op_f32(x.data_ptr(), wp.data_ptr(), _p(bias), _p(alpha_in), _p(alpha_out),
                                                 out.data_ptr(), _p(y2), _p(alpha_dual), B, cin, tin, cout, stride,
                                                 pad, int(output_padding), int(tout_rows), int(tvalid), _stream()),
          "mvq_conv_transpose1d_f32")
    return out if alpha_dual is None else (out, y2)


def pack_segments(z, seg_per_row: int, seg_period: int):
    """z[B, C, T] -> zeros[ceil(B / seg_per_row), C, seg_per_row * seg_period] with item b in columns
    [(b % seg_per_row) * seg_period, ... + T) of row b // seg_per_row (the PACKED latent-rate layout, include/mvq.h)."""
    B, C, T = z.shape
    G = (B + seg_per_row - 1) // seg_per_row
    zp = torch.zeros(G, C, seg_per_row, seg_period, device=z.device, dtype=torch.float32)
    full = B // seg_per_row
    if full:
        zp[:full, :, :, :T] = z[:full * seg_per_row].reshape(full, seg_per_row, C, T).permute(0, 2, 1, 3)
    if B > full * seg_per_row:
        rest = B - full * seg_per_row
        zp[full, :, :rest, :T] = z[full * seg_per_row:].permute(1, 0, 2)
    return zp.reshape(G, C, seg_per_row * seg_period)


def conv1d_packed_rows(xp, wp, cout, ks, seg_per_row, seg_period, seg_valid, bias=None, dil=1, pad=0, residual=None,
                       alpha_out=None, alpha_dual=None, tanh=False):
    """Stride-1 'same' conv on PACKED rows xp[G, cin, seg_per_row * seg_period]; the gap columns of the output are zeros."""
    xp = _dev(xp, "xp")
    G, cin, L = xp.shape
    if L != seg_per_row * seg_period:
        raise MvqError("conv1d_packed_rows: row length != seg_per_row * seg_period")
    out = torch.empty(G, cout, L, device=xp.device, dtype=torch.float32)
    y2 = torch.empty_like(out) if alpha_dual is not None else None
    check(_lib.lib().mvq_conv1d_packed_rows_f32(xp.data_ptr(), wp.data_ptr(), _p(bias), _p(residual), _p(alpha_out), out.data_ptr(),
                                                _p(y2), _p(alpha_dual), G, cin, cout, ks, dil, pad, 1 if tanh else 0,
                                                seg_per_row, seg_period, seg_valid, _stream()), "mvq_conv1d_packed_rows_f32")
    return out if alpha_dual is None else (out, y2)


def vpacked_geometry(tin_rows, tin_valid, ks, stride, dil, pad, follow_pad=0):
    """(tout, tout_rows, per_in) of mvq_conv1d_vpacked_f32 for a conv over x[..., tin_rows] with tin_valid data columns, or None
    when the shape does not qualify.  tout_rows leaves `follow_pad` zero columns behind the valid outputs (the padding the NEXT
    conv needs when it runs on these rows virtually packed too)."""
    tout = conv1d_out_len(tin_valid, ks, stride, dil, pad)
    if tin_rows % 4 or tout <= 0:
        return None
    overhang = (tout - 1) * stride - pad + dil * (ks - 1) - (tin_valid - 1)
    gap = max(pad, overhang, 0)
    tout_rows = (max(tout + follow_pad, -(-(tin_valid + gap) // stride), -(-tin_rows // stride)) + 3) // 4 * 4
    return tout, tout_rows, stride * tout_rows


def conv1d_vpacked(x, wp, cout, ks, seg_per_row, tin_valid, tout_rows, bias=None, stride=1, dil=1, pad=0, residual=None,
                   alpha_out=None, alpha_dual=None, tanh=False):
    """Conv over VIRTUALLY packed rows (include/mvq.h): x[B, cin, tin_rows] with tin_valid data columns + zero tail ->
    y[B, cout, tout_rows] (valid outputs, then zeros).  No copy is made: the kernel's LDS-DMA sources and its stores are remapped."""
    x = _dev(x, "x")
    B, cin, tin_rows = x.shape
    per_in = stride * tout_rows
    out = torch.empty(B, cout, tout_rows, device=x.device, dtype=torch.float32)
    y2 = torch.empty_like(out) if alpha_dual is not None else None
    if residual is not None and tuple(residual.shape) != tuple(out.shape):
        raise MvqError(f"conv1d_vpacked: residual shape {tuple(residual.shape)} != {tuple(out.shape)}")
    check(_lib.lib().mvq_conv1d_vpacked_f32(x.data_ptr(), wp.data_ptr(), _p(bias), _p(residual), _p(alpha_out), out.data_ptr(),
                                            _p(y2), _p(alpha_dual), B, cin, tin_rows, int(tin_valid), cout, ks, stride, dil, pad,
                                            1 if tanh else 0, int(seg_per_row), per_in, tout_rows, _stream()), "mvq_conv1d_vpacked_f32")
    return out if alpha_dual is None else (out, y2)


def conv_transpose1d_packed_rows(xp, wp, cout, stride, pad, seg_per_row, seg_period, seg_valid, batch_out, bias=None,
                                 alpha_in=None, alpha_out=None, alpha_dual=None):
    """ConvTranspose1d(kernel 2*stride, stride, pad) reading PACKED rows, writing the unpacked y[batch_out, cout, Tseg]."""
    xp = _dev(xp, "xp")
    G, cin, L = xp.shape
    if L != seg_per_row * seg_period:
        raise MvqError("conv_transpose1d_packed_rows: row length != seg_per_row * seg_period")
    tout = (seg_valid - 1) * stride - 2 * pad + 2 * stride
    out = torch.empty(batch_out, cout, max(tout, 0), device=xp.device, dtype=torch.float32)
    y2 = torch.empty_like(out) if alpha_dual is not None else None
    check(_lib.lib().mvq_conv_transpose1d_packed_rows_f32(xp.data_ptr(), wp.data_ptr(), _p(bias), _p(alpha_in), _p(alpha_out),
                                                          out.data_ptr(), _p(y2), _p(alpha_dual), G, cin, cout, stride, pad,
                                                          seg_per_row, seg_period, seg_valid, batch_out, _stream()),
          "mvq_conv_transpose1d_packed_rows_f32")
    return out if alpha_dual is None else (out, y2)


def rvq_ema_forward(z, books, n_books_use=None, return_indices=False):
    """ResidualVQEMA.forward.  z[B,D,T]; books[nb,K,D] (stacked).  -> q[B,D,T] (, idx[nb_use, B*T] int64; ``return_indices="int32"``:
    as the kernel wrote them, not widened -- what ops.rvq_rate reads)."""
    z = _dev(z, "z"); books = _dev(books, "books")
    B, D, T = z.shape
    nb_all, K, D2 = books.shape
    if D2 != D:
        raise MvqError(f"rvq: book dim {D2} != token dim {D}")
    nb = nb_all if n_books_use is None else max(0, min(int(n_books_use), nb_all))
    q = torch.empty_like(z)
    idx = torch.empty(nb, B * T, device=z.device, dtype=torch.int32) if return_indices else None
    check(_lib.lib().mvq_rvq_ema_forward_f32(z.data_ptr(), books.data_ptr(), q.data_ptr(), _p(idx), B, D, T, nb, K,
                                             _stream()), "mvq_rvq_ema_forward_f32")
    if return_indices:
        return q, (idx if return_indices == "int32" else idx.long())
    return q


def rvq_ema_step_(z_tokens, books, decay=0.99):
    """ResidualVQEMA.ema_step: updates `books` [nb,K,D] in place."""
    z = _dev(z_tokens, "z_tokens")
    if books.device.type != "cuda" or books.dtype != torch.float32 or not books.is_contiguous():
        raise MvqError("rvq_ema_step_: books must be a contiguous fp32 HIP tensor (updated in place)")
    B, D, T = z.shape
    nb, K, _ = books.shape
    nbytes = _lib.lib().mvq_rvq_ema_step_scratch_bytes(B, T, nb, K, D)
    scratch = torch.empty(max(nbytes, 4), device=z.device, dtype=torch.uint8)
    check(_lib.lib().mvq_rvq_ema_step_f32(z.data_ptr(), books.data_ptr(), scratch.data_ptr(), B, D, T, nb, K,
                                          float(decay), _stream()), "mvq_rvq_ema_step_f32")
    return books


def dac_rvq_prepare(codebook):
    """F.normalize(codebook[nq, K, Dc]) and its squared norms, once (model load): -> (cb_normalised, cb_norm2) for dac_rvq."""
    codebook = _dev(codebook, "codebook")
    nq, K, Dc = codebook.shape
    cbn = torch.empty_like(codebook)
    cn2 = torch.empty(nq, K, device=codebook.device, dtype=torch.float32)
    check(_lib.lib().mvq_dac_rvq_prepare_f32(codebook.data_ptr(), cbn.data_ptr(), cn2.data_ptr(), nq, K, Dc, _stream()),
          "mvq_dac_rvq_prepare_f32")
    return cbn, cn2


def dac_rvq(z, in_w, in_b, codebook, out_w, out_b, n_q, nq_item=None, prepared=None):
    """DAC ResidualVectorQuantize -> (z_q, codes int64 [B,nq,T], latents [B,nq*Dc,T]).  ``nq_item`` (int32 [B] on the
    device): train-mode quantiser dropout -- item b's z_q sums only its first nq_item[b] stages.  ``prepared`` =
    dac_rvq_prepare(codebook): the normalised codebook computed once instead of in every block (same results)."""
    z = _dev(z, "z")
    B, C, T = z.shape
    _, K, Dc = codebook.shape
    zq = torch.empty_like(z)
    codes = torch.empty(B, n_q, T, device=z.device, dtype=torch.int32)
    lat = torch.empty(B, n_q * Dc, T, device=z.device, dtype=torch.float32)
    if nq_item is not None and (nq_item.dtype != torch.int32 or nq_item.numel() != B or not nq_item.is_cuda):
        raise MvqError("dac_rvq: nq_item must be an int32 HIP tensor with one entry per batch item")
    cbn, cn2 = prepared if prepared is not None else (None, None)
    check(_lib.lib().mvq_dac_rvq_prepared_f32(z.data_ptr(), in_w.data_ptr(), in_b.data_ptr(), codebook.data_ptr(), _p(cbn), _p(cn2),
                                              out_w.data_ptr(), out_b.data_ptr(), zq.data_ptr(), codes.data_ptr(),
                                              lat.data_ptr(), _p(nq_item), B, C, T, n_q, K, Dc, _stream()), "mvq_dac_rvq_f32")
    return zq, codes.long(), lat


def _codes_i64(x, name):
    if not isinstance(x, torch.Tensor) or x.device.type != "cuda":
        raise MvqError(f"{name}: expected an integer tensor on a HIP device")
    if x.dtype.is_floating_point or x.dtype == torch.bool:
        raise MvqError(f"{name}: expected an integer tensor, got {x.dtype}")
    return x.to(torch.int64).contiguous()


def rvq_dequant(idx, books, n_books_use=None, out=None, out_strides=None):
    """The receiver side of ResidualVQEMA: idx[nb, B, T] (int) -> q[B, D, T] = e_0[idx_0] + e_1[idx_1] + ... (book order, from +0).
    ``out`` / ``out_strides`` = (batch stride, dim stride): write into another layout instead (token-folded [1, D, B*T] is
    (T, B*T)).  Indices are clamped to [0, K) in the kernel; validate untrusted ones on the host (bitstream.unpack_indices)."""
    idx = _codes_i64(idx, "idx"); books = _dev(books, "books")
    if idx.dim() != 3:
        raise MvqError(f"rvq_dequant: idx must be [n_books, B, T], got {tuple(idx.shape)}")
    if books.dim() != 3 or idx.device != books.device:
        raise MvqError("rvq_dequant: books must be [n_books, K, D] on idx's device")
    nb_all, K, D = books.shape
    nb = min(idx.shape[0], nb_all) if n_books_use is None else max(0, min(int(n_books_use), idx.shape[0], nb_all))
    _, B, T = idx.shape
    if out is None:
        out = torch.empty(B, D, T, device=books.device, dtype=torch.float32)
        out_strides = (D * T, T)
    elif (not isinstance(out, torch.Tensor) or out.device != books.device or out.dtype != torch.float32
          or not out.is_contiguous() or out_strides is None):
        raise MvqError("rvq_dequant: out must be a contiguous fp32 tensor on the books' device, given with out_strides")
    sb, sd = int(out_strides[0]), int(out_strides[1])
    if sb < 0 or sd < 0 or (B and T and (B - 1) * sb + (D - 1) * sd + T > out.numel()):
        raise MvqError(f"rvq_dequant: [B={B}, D={D}, T={T}] at strides ({sb}, {sd}) reaches past the {out.numel()}-element out")
    check(_lib.lib().mvq_rvq_dequant_f32(idx.data_ptr(), books.data_ptr(), out.data_ptr(), B, D, T, nb, K,
                                         sb, sd, _stream()), "mvq_rvq_dequant_f32")
    return out


def _nb_valid_u8(nb_valid, B, T, device, name, arg="nb_valid", of="idx"):
    if not isinstance(nb_valid, torch.Tensor) or nb_valid.device != device:
        raise MvqError(f"{name}: {arg} must be a tensor on the device of {of}")
    if nb_valid.dtype != torch.uint8 or tuple(nb_valid.shape) != (B, T):
        raise MvqError(f"{name}: {arg} must be uint8 [B={B}, T={T}], got {nb_valid.dtype} {tuple(nb_valid.shape)}")
    return nb_valid.contiguous()


def rvq_dequant_layers(idx, books, nb_valid, n_books_use=None, out=None, out_strides=None):
    """rvq_dequant with a per-token book count: token (b, t) sums its first min(n_books_use, nb_valid[b, t]) books (a count of 0
    gives +0: a lost token).  nb_valid: uint8 [B, T] on the device, or None (= rvq_dequant)."""
    if nb_valid is None:
        return rvq_dequant(idx, books, n_books_use, out=out, out_strides=out_strides)
    idx = _codes_i64(idx, "idx"); books = _dev(books, "books")
    if idx.dim() != 3:
        raise MvqError(f"rvq_dequant_layers: idx must be [n_books, B, T], got {tuple(idx.shape)}")
    if books.dim() != 3 or idx.device != books.device:
        raise MvqError("rvq_dequant_layers: books must be [n_books, K, D] on idx's device")
    nb_all, K, D = books.shape
    nb = min(idx.shape[0], nb_all) if n_books_use is None else max(0, min(int(n_books_use), idx.shape[0], nb_all))
    _, B, T = idx.shape
    nbv = _nb_valid_u8(nb_valid, B, T, idx.device, "rvq_dequant_layers")
    if out is None:
        out = torch.empty(B, D, T, device=books.device, dtype=torch.float32)
        out_strides = (D * T, T)
    elif (not isinstance(out, torch.Tensor) or out.device != books.device or out.dtype != torch.float32
          or not out.is_contiguous() or out_strides is None):
        raise MvqError("rvq_dequant_layers: out must be a contiguous fp32 tensor on the books' device, given with out_strides")
    sb, sd = int(out_strides[0]), int(out_strides[1])
    if sb < 0 or sd < 0 or (B and T and (B - 1) * sb + (D - 1) * sd + T > out.numel()):
        raise MvqError(f"rvq_dequant_layers: [B={B}, D={D}, T={T}] at strides ({sb}, {sd}) reaches past the {out.numel()}-element out")
    check(_lib.lib().mvq_rvq_dequant_layers_f32(idx.data_ptr(), books.data_ptr(), nbv.data_ptr(), out.data_ptr(), B, D, T, nb, K,
                                                sb, sd, _stream()), "mvq_rvq_dequant_layers_f32")
    return out


def rvq_rate(z, idx, books, rate, packet_tok, n_books_use=None, folded_batch=None, nb_valid_out=None, nb_sent_out=None, col=0,
             want_energy=False, group_tok=16):
    """Closed-loop sender rate control on the search's result (mvq_rvq_rate_f32): decide how many books each packet carries and
    sum exactly those, in the receiver's arithmetic.  z[B, D, T] (or token-folded [1, D, B*T] with ``folded_batch`` = B), idx
    [nb, B, T] / [nb, B*T] (int32 as the search writes it, or int64) of rvq_ema_forward on that z, books[nb_all, K, D]; ``rate`` a
    packets.Rate.  Groups of ``group_tok`` tokens start at token 0 of each item.  -> (q shaped and laid out like z, nb_valid uint8
    [B, T], nb_sent uint8 [B, P]) and energy fp32 [nb + 1, B*T] with ``want_energy``.  ``nb_valid_out`` [B, W] / ``nb_sent_out``
    [B, Wp] (uint8, contiguous): write the counts there instead, tokens from column ``col`` and packets from col // packet_tok
    (a chunk of a longer item); they are returned as given."""
    z = _dev(z, "z"); books = _dev(books, "books")
    if z.dim() != 3 or books.dim() != 3 or books.device != z.device or books.shape[2] != z.shape[1]:
        raise MvqError(f"rvq_rate: z {tuple(z.shape)} and books {tuple(books.shape)} must be [B, D, T] and [n_books, K, D] on one device")
    D = z.shape[1]
    if folded_batch is None:
        B, T = z.shape[0], z.shape[2]
        z_sb, z_sd = D * T, T
    else:
        B = int(folded_batch)
        if z.shape[0] != 1 or B < 1 or z.shape[2] % B:
            raise MvqError(f"rvq_rate: z {tuple(z.shape)} is not token-folded [1, D, {B}*T]")
        T = z.shape[2] // B
        z_sb, z_sd = T, B * T
    nb_all, K, _ = books.shape
    if not isinstance(idx, torch.Tensor) or idx.device != z.device or idx.dtype not in (torch.int32, torch.int64):
        raise MvqError("rvq_rate: idx must be an int32 or int64 tensor on z's device")
    if idx.dim() not in (2, 3) or idx.numel() != idx.shape[0] * B * T:
        raise MvqError(f"rvq_rate: idx {tuple(idx.shape)} for [n_books, B={B}, T={T}]")
    nb = min(idx.shape[0], nb_all) if n_books_use is None else max(0, min(int(n_books_use), idx.shape[0], nb_all))
    idx = idx.to(torch.int32).contiguous()
    packet_tok, col = int(packet_tok), int(col)
    min_books, mode, tol2, budget = rate.resolve(nb, packet_tok, group_tok)
    if col < 0 or col % int(group_tok):
        raise MvqError(f"rvq_rate: col = {col} is not the start of a {group_tok}-token group")
    P = (T + packet_tok - 1) // packet_tok
    outs = []
    for t, name, n, c in ((nb_valid_out, "nb_valid_out", T, col), (nb_sent_out, "nb_sent_out", P, col // packet_tok)):
        if t is None:
            t, c = torch.empty(B, n, device=z.device, dtype=torch.uint8), 0
        elif (not isinstance(t, torch.Tensor) or t.device != z.device or t.dtype != torch.uint8 or t.dim() != 2 or t.shape[0] != B
              or not t.is_contiguous() or c + n > t.shape[1]):
            raise MvqError(f"rvq_rate: {name} must be a contiguous uint8 tensor [B={B}, >= {c + n}] on z's device")
        outs.append((t, c))
    (nbv, cv), (nbs, cs) = outs
    q = torch.empty_like(z)
    energy = torch.empty(nb + 1, B * T, device=z.device, dtype=torch.float32) if want_energy else None
    check(_lib.lib().mvq_rvq_rate_f32(z.data_ptr(), z_sb, z_sd, idx.data_ptr(), B * T, T, books.data_ptr(), q.data_ptr(), z_sb, z_sd,
                                      nbv.data_ptr() + cv, nbv.shape[1], nbs.data_ptr() + cs, nbs.shape[1], _p(energy), B, D, T, nb, K,
                                      packet_tok, int(group_tok), min_books, mode, tol2, budget, _stream()), "mvq_rvq_rate_f32")
    return (q, nbv, nbs, energy) if want_energy else (q, nbv, nbs)


def rvq_beam(z, books, beam, n_books_use=None, folded_batch=None, valid=None, want_slot=False, want_energy=False):
    """Beam search over the books at the sender (mvq_rvq_beam_f32): ``beam`` (1..8) paths per token instead of
    the greedy one, the path with the smallest final residual energy is returned; ``beam`` = 1 gives ops.rvq_ema_forward's indices.
    z[B, D, T], token-folded [1, D, B*T] with ``folded_batch`` = B, or the staged loop's [B, D, W] with ``valid`` = the T <= W
    tokens of each item that count; books[nb_all, K, D].  -> idx int32 [nb, B*T] (what ops.rvq_rate reads; token b*T + t), then
    with ``want_slot`` the winning slot uint8 [B*T] (0: the greedy path won) and with ``want_energy`` the winner's final residual
    energy fp32 [B*T]."""
    z = _dev(z, "z"); books = _dev(books, "books")
    if z.dim() != 3 or books.dim() != 3 or books.device != z.device or books.shape[2] != z.shape[1]:
        raise MvqError(f"rvq_beam: z {tuple(z.shape)} and books {tuple(books.shape)} must be [B, D, T] and [n_books, K, D] on one device")
    if isinstance(beam, bool) or int(beam) != beam:
        raise MvqError(f"rvq_beam: beam = {beam!r} is not an integer")
    D = z.shape[1]
    if folded_batch is None:
        B, W = z.shape[0], z.shape[2]
        T = W if valid is None else int(valid)
        if not 0 <= T <= W:
            raise MvqError(f"rvq_beam: valid = {valid!r} outside 0..{W}")
        z_sb, z_sd = D * W, W
    else:
        B = int(folded_batch)
        if valid is not None or z.shape[0] != 1 or B < 1 or z.shape[2] % B:
            raise MvqError(f"rvq_beam: z {tuple(z.shape)} is not token-folded [1, D, {B}*T] (and takes no valid=)")
        T = z.shape[2] // B
        z_sb, z_sd = T, B * T
    nb_all, K, _ = books.shape
    nb = nb_all if n_books_use is None else max(0, min(int(n_books_use), nb_all))
    idx = torch.empty(nb, B * T, device=z.device, dtype=torch.int32)
    slot = torch.empty(B * T, device=z.device, dtype=torch.uint8) if want_slot else None
    energy = torch.empty(B * T, device=z.device, dtype=torch.float32) if want_energy else None
    check(_lib.lib().mvq_rvq_beam_f32(z.data_ptr(), z_sb, z_sd, books.data_ptr(), idx.data_ptr(), B * T, T, _p(slot), _p(energy), B, D, T,
                                      nb, K, int(beam), _stream()), "mvq_rvq_beam_f32")
    out = (idx,) + ((slot,) if want_slot else ()) + ((energy,) if want_energy else ())
    return out[0] if len(out) == 1 else out


PACKET_MAX_BITS = 24           # the packet kernels cover ceil(log2 K) <= 24, nb and packet_tok <= 255 (include/mvq.h)


def _packet_shape(name, k, nb, T, packet_tok):
    """(P, body_full) after the checks the C ABI repeats."""
    from .packets import body_bytes, n_packets
    from .bitstream import index_bits
    k, nb, T, packet_tok = int(k), int(nb), int(T), int(packet_tok)
    if k < 1 or index_bits(k) > PACKET_MAX_BITS or not 0 <= nb <= 255 or T < 0 or not 1 <= packet_tok <= 255:
        raise MvqError(f"{name}: K={k}, nb={nb}, T={T}, packet_tok={packet_tok} outside the packet kernels "
                       f"(ceil(log2 K) <= {PACKET_MAX_BITS}, nb <= 255, 1 <= packet_tok <= 255)")
    return n_packets(T, packet_tok), body_bytes(packet_tok, nb, k)


def idx_pack_packets(idx, k, packet_tok, book_dim=0):
    """Indices -> packet bodies uint8 [B, P, body_full] (packets.py's pack_bodies per item, bit for bit; indices clamped to
    [0, K)).  idx is [nb, B, T] (``book_dim=0``, the RVQ indices) or [B, nb, T] (``book_dim=1``, DAC codes); read in place."""
    idx = _codes_i64(idx, "idx")
    if idx.dim() != 3 or book_dim not in (0, 1):
        raise MvqError(f"idx_pack_packets: idx must be [nb, B, T] (book_dim=0) or [B, nb, T] (book_dim=1), got {tuple(idx.shape)}")
    if book_dim == 0:
        nb, B, T = idx.shape
        s_book, s_item = B * T, T
    else:
        B, nb, T = idx.shape
        s_book, s_item = T, nb * T
    P, full = _packet_shape("idx_pack_packets", k, nb, T, packet_tok)
    bodies = torch.empty(B, P, full, device=idx.device, dtype=torch.uint8)
    check(_lib.lib().mvq_idx_pack_packets_u8(idx.data_ptr(), bodies.data_ptr(), B, nb, T, int(k), int(packet_tok), s_book, s_item,
                                             _stream()), "mvq_idx_pack_packets_u8")
    return bodies


def idx_unpack_packets(bodies, nb_recv, k, nb, T, packet_tok):
    """bodies uint8 [B, P, body_full] and nb_recv uint8 [B, P] (books of each packet that arrived, 0 = lost) ->
    (idx int64 [nb, B, T], nb_valid uint8 [B, T]): packets.py's unpack_bodies per item, bit for bit."""
    for t, name in ((bodies, "bodies"), (nb_recv, "nb_recv")):
        if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
            raise MvqError(f"idx_unpack_packets: {name} must be a uint8 tensor on a HIP device")
        if t.dtype != torch.uint8:
            raise MvqError(f"idx_unpack_packets: {name} must be uint8, got {t.dtype}")
    P, full = _packet_shape("idx_unpack_packets", k, nb, T, packet_tok)
    if bodies.dim() != 3 or tuple(bodies.shape[1:]) != (P, full):
        raise MvqError(f"idx_unpack_packets: bodies {tuple(bodies.shape)} for [B, P={P}, body_full={full}]")
    B = bodies.shape[0]
    if nb_recv.device != bodies.device or tuple(nb_recv.shape) != (B, P):
        raise MvqError(f"idx_unpack_packets: nb_recv {tuple(nb_recv.shape)} for [B={B}, P={P}] on the device of bodies")
    bodies, nb_recv = bodies.contiguous(), nb_recv.contiguous()
    idx = torch.empty(int(nb), B, int(T), device=bodies.device, dtype=torch.int64)
    nb_valid = torch.empty(B, int(T), device=bodies.device, dtype=torch.uint8)
    check(_lib.lib().mvq_idx_unpack_packets(bodies.data_ptr(), nb_recv.data_ptr(), idx.data_ptr(), nb_valid.data_ptr(), B, int(nb),
                                            int(T), int(k), int(packet_tok), _stream()), "mvq_idx_unpack_packets")
    return idx, nb_valid


def _fec_shape(name, info, fec):
    """(K, nb, T, packet_tok, P, body_full, g, m, G, W, r, the shape of one item's parity rows) after the checks the C ABI
    repeats: (G, g + W) for r == 1, (G, r, g + W) for the Reed-Solomon code."""
    from .packets import StreamInfo
    try:
        info = StreamInfo(*(int(v) for v in info))
        g, m, r = int(fec.group), int(fec.books), int(fec.parity)
    except (TypeError, ValueError, AttributeError) as e:
        raise MvqError(f"{name}: info must be a packets.StreamInfo and fec a packets.Fec ({e})") from None
    P, full = _packet_shape(name, info.K, info.nb, info.T, info.packet_tok)
    if not 1 <= g <= 16 or not 1 <= m <= info.nb or not 1 <= r <= 4:
        raise MvqError(f"{name}: Fec(group={g}, books={m}, parity={r}) outside group 1..16, books 1..nb = {info.nb}, parity 1..4")
    from .packets import body_bytes
    G, W = (P + g - 1) // g, body_bytes(info.packet_tok, m, info.K)
    return info.K, info.nb, info.T, info.packet_tok, P, full, g, m, G, W, r, ((G, g + W) if r == 1 else (G, r, g + W))


def _fec_u8(name, what, t, shape, dev=None, contiguous=False):
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda" or t.dtype != torch.uint8:
        raise MvqError(f"{name}: {what} must be a uint8 tensor on a HIP device")
    if (dev is not None and t.device != dev) or t.dim() != len(shape) or any(w is not None and int(v) != w for v, w in zip(t.shape, shape)):
        raise MvqError(f"{name}: {what} {tuple(t.shape)} for {list(shape)} on the device of bodies")
    if contiguous and not t.is_contiguous():
        raise MvqError(f"{name}: {what} is written in place and must be contiguous")
    return t if contiguous else t.contiguous()


def fec_parity(bodies, nb_sent, info, fec):
    """bodies uint8 [B, P, body_full] and nb_sent uint8 [B, P] (None: every packet carries info.nb books) -> the parity rows uint8
    [B, G, g + W]: packets.fec_rows per item, bit for bit (mvq_fec_parity_u8).  With fec.parity = r > 1 the Reed-Solomon rows uint8
    [B, G, r, g + W] (mvq_fec_rs_parity_u8)."""
    K, nb, T, ptok, P, full, g, m, G, W, r, rshape = _fec_shape("fec_parity", info, fec)
    bodies = _fec_u8("fec_parity", "bodies", bodies, (None, P, full))
    B = bodies.shape[0]
    if nb_sent is not None:
        nb_sent = _fec_u8("fec_parity", "nb_sent", nb_sent, (B, P), bodies.device)
    rows = torch.empty(B, *rshape, device=bodies.device, dtype=torch.uint8)
    if r == 1:
        check(_lib.lib().mvq_fec_parity_u8(bodies.data_ptr(), _p(nb_sent), rows.data_ptr(), B, nb, T, K, ptok, g, m, _stream()),
              "mvq_fec_parity_u8")
    else:
        check(_lib.lib().mvq_fec_rs_parity_u8(bodies.data_ptr(), _p(nb_sent), rows.data_ptr(), B, nb, T, K, ptok, g, m, r, _stream()),
              "mvq_fec_rs_parity_u8")
    return rows


def fec_recover(bodies, nb_recv, rows, got, info, fec, want_recovered=False):
    """packets.fec_recover per item on the device, IN PLACE on bodies uint8 [B, P, body_full] and nb_recv uint8 [B, P] (both
    contiguous), from the parity rows uint8 [B, G, g + W] and got uint8 [B, G] (0 = the group's parity did not arrive): where
    exactly one packet of a group is deficient it is rebuilt to its protected books (mvq_fec_recover_u8).  With fec.parity = r > 1:
    rows uint8 [B, G, r, g + W] and got a bitmask (bit i: parity i of the group arrived); any d <= (arrived parities) deficient
    packets of a group are rebuilt together (mvq_fec_rs_recover_u8).
    -> (bodies, nb_recv), with ``want_recovered`` also recovered uint8 [B, P]."""
    K, nb, T, ptok, P, full, g, m, G, W, r, rshape = _fec_shape("fec_recover", info, fec)
    bodies = _fec_u8("fec_recover", "bodies", bodies, (None, P, full), contiguous=True)
    B = bodies.shape[0]
    nb_recv = _fec_u8("fec_recover", "nb_recv", nb_recv, (B, P), bodies.device, contiguous=True)
    rows = _fec_u8("fec_recover", "rows", rows, (B, *rshape), bodies.device)
    got = _fec_u8("fec_recover", "got", got, (B, G), bodies.device)
    recovered = torch.empty(B, P, device=bodies.device, dtype=torch.uint8) if want_recovered else None
    if r == 1:
        check(_lib.lib().mvq_fec_recover_u8(bodies.data_ptr(), nb_recv.data_ptr(), rows.data_ptr(), got.data_ptr(), _p(recovered), B, nb, T,
                                            K, ptok, g, m, _stream()), "mvq_fec_recover_u8")
    else:
        check(_lib.lib().mvq_fec_rs_recover_u8(bodies.data_ptr(), nb_recv.data_ptr(), rows.data_ptr(), got.data_ptr(), _p(recovered), B, nb,
                                               T, K, ptok, g, m, r, _stream()), "mvq_fec_rs_recover_u8")
    return (bodies, nb_recv, recovered) if want_recovered else (bodies, nb_recv)


def dac_rvq_from_codes(codes, codebook, out_w, out_b, want_z_p=True, nq_valid=None):
    """upstream ResidualVectorQuantize.from_codes: codes[B, nq, T] (int) -> (z_q [B,C,T], z_p [B,nq*Dc,T] or None).
    z_q = sum over stages of out_proj_i(codebook_i[code_i]) in stage order; the first nq stages of the stacked weights.
    ``nq_valid`` (uint8 [B, T] on the device; None = every stage, today's launch): token (b, t) sums only its first
    min(nq, nq_valid[b, t]) stages -- what arrived of a layered audio packet; 0 gives +0 in every channel
    (mvq_dac_rvq_from_codes_layers_f32).  z_p holds the raw rows of all nq stages either way."""
    codes = _codes_i64(codes, "codes"); codebook = _dev(codebook, "codebook")
    out_w = _dev(out_w, "out_w"); out_b = _dev(out_b, "out_b")
    if codes.dim() != 3 or codebook.dim() != 3 or out_w.dim() != 3 or out_b.dim() != 2:
        raise MvqError("dac_rvq_from_codes: codes [B,nq,T], codebook [nq,K,Dc], out_w [nq,C,Dc], out_b [nq,C] expected")
    if len({codes.device, codebook.device, out_w.device, out_b.device}) != 1:
        raise MvqError("dac_rvq_from_codes: all tensors must be on one device")
    B, nq, T = codes.shape
    _, K, Dc = codebook.shape
    C = out_w.shape[1]
    if nq > min(codebook.shape[0], out_w.shape[0], out_b.shape[0]):
        raise MvqError(f"dac_rvq_from_codes: {nq} code rows for {codebook.shape[0]} codebooks / {out_w.shape[0]} out_w / "
                       f"{out_b.shape[0]} out_b stages")
    if out_w.shape[2] != Dc or out_b.shape[1] != C:
        raise MvqError(f"dac_rvq_from_codes: out_w {tuple(out_w.shape)} / out_b {tuple(out_b.shape)} do not match Dc={Dc}, C={C}")
    zq = torch.empty(B, C, T, device=codes.device, dtype=torch.float32)
    z_p = torch.empty(B, nq * Dc, T, device=codes.device, dtype=torch.float32) if want_z_p else None
    if nq == 0:
        zq.zero_()
        return zq, z_p
    if nq_valid is not None:
        nqv = _nb_valid_u8(nq_valid, B, T, codes.device, "dac_rvq_from_codes", arg="nq_valid", of="codes")
        check(_lib.lib().mvq_dac_rvq_from_codes_layers_f32(codes.data_ptr(), nq * T, codebook.data_ptr(), out_w.data_ptr(),
                                                           out_b.data_ptr(), nqv.data_ptr(), zq.data_ptr(), _p(z_p), B, C, T, nq, K, Dc,
                                                           _stream()), "mvq_dac_rvq_from_codes_layers_f32")
        return zq, z_p
    check(_lib.lib().mvq_dac_rvq_from_codes_f32(codes.data_ptr(), codebook.data_ptr(), out_w.data_ptr(), out_b.data_ptr(),
                                                zq.data_ptr(), _p(z_p), B, C, T, nq, K, Dc, _stream()), "mvq_dac_rvq_from_codes_f32")
    return zq, z_p


def dac_rvq_rate(z, codes, codebook, out_w, out_b, rate, packet_tok, na_use=None, want_energy=False):
    """Closed-loop audio rate control on the DAC quantiser's result (mvq_dac_rvq_rate_f32): decide how many stages each audio packet
    carries and sum exactly those, in the receiver's arithmetic (dac_rvq_from_codes(nq_valid=)).  z[B, C, T] fp32 (the encoder
    output the quantiser searched), codes[B, nq, T] int64 of dac_rvq on that z (the first ``na_use`` rows are read in place),
    the stacked weights as dac_rvq_from_codes takes them; ``rate`` a packets.Rate.  Groups of 16 tokens start at token 0 of each
    item.  -> (qa [B, C, T], na_valid uint8 [B, T], na_sent uint8 [B, P]) and energy fp32 [na_use + 1, B*T] with ``want_energy``."""
    from .packets import Rate
    if not isinstance(rate, Rate):
        raise ValueError(f"dac_rvq_rate: rate must be a packets.Rate, not {type(rate).__name__}")
    z = _dev(z, "z"); codes = _codes_i64(codes, "codes"); codebook = _dev(codebook, "codebook")
    out_w = _dev(out_w, "out_w"); out_b = _dev(out_b, "out_b")
    if z.dim() != 3 or codes.dim() != 3 or codebook.dim() != 3 or out_w.dim() != 3 or out_b.dim() != 2:
        raise MvqError("dac_rvq_rate: z [B,C,T], codes [B,nq,T], codebook [nq,K,Dc], out_w [nq,C,Dc], out_b [nq,C] expected")
    if len({z.device, codes.device, codebook.device, out_w.device, out_b.device}) != 1:
        raise MvqError("dac_rvq_rate: all tensors must be on one device")
    B, C, T = z.shape
    _, K, Dc = codebook.shape
    stages = min(codes.shape[1], codebook.shape[0], out_w.shape[0], out_b.shape[0])
    na = stages if na_use is None else int(na_use)
    if codes.shape[0] != B or codes.shape[2] != T or out_w.shape[1] != C or out_w.shape[2] != Dc or out_b.shape[1] != C:
        raise MvqError(f"dac_rvq_rate: z {tuple(z.shape)}, codes {tuple(codes.shape)}, out_w {tuple(out_w.shape)}, out_b "
                       f"{tuple(out_b.shape)} do not describe one [B, C, T] with Dc={Dc}")
    if not 1 <= na <= stages:
        raise MvqError(f"dac_rvq_rate: na_use = {na} outside 1..{stages} (the stages the codes and weights have)")
    if C % 64 or Dc != 8 or na > 32:
        raise MvqError(f"dac_rvq_rate: C={C}, Dc={Dc}, na_use={na} outside the kernels (C % 64 == 0, Dc = 8, na_use <= 32)")
    packet_tok = int(packet_tok)
    min_books, mode, tol2, budget = rate.resolve(na, packet_tok, 16)
    P = (T + packet_tok - 1) // packet_tok
    dev = z.device
    qa = torch.empty(B, C, T, device=dev, dtype=torch.float32)
    na_valid = torch.empty(B, T, device=dev, dtype=torch.uint8)
    na_sent = torch.empty(B, P, device=dev, dtype=torch.uint8)
    energy = torch.empty(na + 1, B * T, device=dev, dtype=torch.float32) if want_energy else None
    if B and T:
        nbytes = _lib.lib().mvq_dac_rvq_rate_workspace_bytes(B, C, T, na)
        work = torch.empty(max(nbytes // 4, 4), device=dev, dtype=torch.float32)
        check(_lib.lib().mvq_dac_rvq_rate_f32(z.data_ptr(), codes.data_ptr(), codes.shape[1] * T, codebook.data_ptr(), out_w.data_ptr(),
                                              out_b.data_ptr(), qa.data_ptr(), na_valid.data_ptr(), na_sent.data_ptr(), _p(energy),
                                              work.data_ptr(), work.numel() * 4, B, C, T, na, K, Dc, packet_tok, min_books, mode, tol2,
                                              budget, _stream()), "mvq_dac_rvq_rate_f32")
    return (qa, na_valid, na_sent, energy) if want_energy else (qa, na_valid, na_sent)


def layernorm_c(x, gamma, beta, pe=None, eps=1e-5, do_tanh=False, post_scale=1.0, folded_batch=None, sub=None):
    """LayerNorm over channels of x[B,C,T] (of x - sub when ``sub`` is given); with ``folded_batch=B`` x is the
    token-folded [1,C,B*T] layout."""
    x = _dev(x, "x")
    if sub is not None:
        sub = _dev(sub, "sub")
        if sub.shape != x.shape:
            raise MvqError("layernorm_c: sub must have the shape of x")
    B, C, T = x.shape
    sb = sc = 0
    if folded_batch is not None:
        if B != 1 or T % folded_batch:
            raise MvqError("layernorm_c: folded tensor must be [1, C, B*T]")
        B, T = folded_batch, T // folded_batch
        sb, sc = T, B * T
    y = torch.empty_like(x)
    if pe is not None and (pe.shape[0] < T or pe.shape[1] != C):
        raise MvqError(f"layernorm_c: pe table {tuple(pe.shape)} too small for T={T}, C={C}")
    check(_lib.lib().mvq_layernorm_c_sub_f32(x.data_ptr(), _p(sub), _p(pe), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(),
                                             B, C, T, sb, sc, float(eps), int(do_tanh), float(post_scale), _stream()),
          "mvq_layernorm_c_f32")
    return y


def _chunk_key_mask(who, kmask, m_stride, B, Tk, device):
    """The flat uint8 key mask of a chunk call (item b's key j at b*m_stride + j, m_stride defaults to Tk) -> (kmask, m_stride)."""
    kmask = _key_mask_u8(who, kmask, device)
    ms = int(Tk if m_stride is None else m_stride)
    if ms < 0 or (B and Tk and (B - 1) * ms + Tk > kmask.numel()):
        raise MvqError(f"{who}: an item's mask row reaches past the end of kmask ({kmask.numel()} entries, B={B}, Tk={Tk}, m_stride={ms})")
    return kmask, ms


def attention(q, k, v, heads, folded_batch=None, kmask=None, m_stride=None):
    """``kmask`` (uint8 on the device, nonzero = key present; item b's key j at b*m_stride + j, ``m_stride`` defaults to Tk, so a
    contiguous [B, Tk] mask serves the plain and the token-folded layout alike): mvq_attention_masked_f32."""
    q = _dev(q, "q"); k = _dev(k, "k"); v = _dev(v, "v")
    B, C, Tq = q.shape
    Tk = k.shape[2]
    strides = (0, 0, 0, 0)
    if folded_batch is not None:
        B = folded_batch
        Tq, Tk = Tq // B, Tk // B
        strides = (Tq, B * Tq, Tk, B * Tk)
    ctx = torch.empty_like(q)
    if kmask is not None:
        kmask, ms = _chunk_key_mask("attention", kmask, m_stride, B, Tk, q.device)
        check(_lib.lib().mvq_attention_masked_f32(q.data_ptr(), k.data_ptr(), v.data_ptr(), kmask.data_ptr(), ctx.data_ptr(), B, heads,
                                                  C // heads, Tq, Tk, *strides, ms, _stream()), "mvq_attention_masked_f32")
        return ctx
    check(_lib.lib().mvq_attention_f32(q.data_ptr(), k.data_ptr(), v.data_ptr(), ctx.data_ptr(), B, heads, C // heads,
                                       Tq, Tk, *strides, _stream()), "mvq_attention_f32")
    return ctx


def attention_kv_slice(q, k_all, v_all, heads, folded_batch, s, tk):
    """Attention of token-folded q[1,C,B*Tq] against columns [s, s+tk) of token-folded K/V over the WHOLE sequence
    (k_all, v_all: [1, C, B*Ta], column b*Ta + t): the kernel takes strides, nothing is copied."""
    q = _dev(q, "q"); k_all = _dev(k_all, "k"); v_all = _dev(v_all, "v")
    B = folded_batch
    C, Tq, Ta = q.shape[1], q.shape[2] // B, k_all.shape[2] // B
    if s < 0 or tk < 0 or s + tk > Ta:
        raise MvqError("attention_kv_slice: slice outside the key/value sequence")
    ctx = torch.empty_like(q)
    check(_lib.lib().mvq_attention_f32(q.data_ptr(), k_all.data_ptr() + 4 * s, v_all.data_ptr() + 4 * s, ctx.data_ptr(),
                                       B, heads, C // heads, Tq, tk, Tq, B * Tq, Ta, B * Ta, _stream()), "mvq_attention_f32")
    return ctx


def _key_mask_u8(who, kmask, device):
    if not isinstance(kmask, torch.Tensor) or kmask.device != device or kmask.dtype != torch.uint8 or not kmask.is_contiguous():
        raise MvqError(f"{who}: kmask must be a contiguous uint8 tensor on the device of q (nonzero = key present)")
    return kmask


def attention_into_(ctx, q, k, v, heads, batch, tq, tk, q_strides, k_strides, q_col=0, k_col=0, kmask=None, m_stride=None):
    """ctx = attention of ``batch`` query groups against their own key groups, on views of token-folded [1, C, N] tensors:
    group g's query column i / channel c sits at q_col + g*q_strides[0] + c*q_strides[1] + i (ctx shares that addressing),
    its keys likewise from k_col with k_strides.  Writes into ``ctx`` (the receiver's chunk-as-batch calls).
    ``kmask`` (flat uint8 on the device, nonzero = key present): group g's key j is masked by kmask[k_col + g*m_stride + j]
    (``m_stride`` defaults to k_strides[0]): mvq_attention_masked_f32, an absent key is not a key."""
    C = q.shape[1]
    if batch and tq and (q_col + (batch - 1) * q_strides[0] + (C - 1) * q_strides[1] + tq > q.numel()
                         or (tk and k_col + (batch - 1) * k_strides[0] + (C - 1) * k_strides[1] + tk > k.numel())):
        raise MvqError("attention_into_: a group reaches past the end of its tensor")
    if kmask is not None:
        kmask = _key_mask_u8("attention_into_", kmask, q.device)
        ms = int(k_strides[0] if m_stride is None else m_stride)
        if batch and tk and k_col + (batch - 1) * ms + tk > kmask.numel():
            raise MvqError("attention_into_: a group's mask row reaches past the end of kmask")
        check(_lib.lib().mvq_attention_masked_f32(q.data_ptr() + 4 * q_col, k.data_ptr() + 4 * k_col, v.data_ptr() + 4 * k_col,
                                                  kmask.data_ptr() + k_col, ctx.data_ptr() + 4 * q_col, batch, heads, C // heads,
                                                  tq, tk, int(q_strides[0]), int(q_strides[1]), int(k_strides[0]),
                                                  int(k_strides[1]), ms, _stream()), "mvq_attention_masked_f32")
        return ctx
    check(_lib.lib().mvq_attention_f32(q.data_ptr() + 4 * q_col, k.data_ptr() + 4 * k_col, v.data_ptr() + 4 * k_col,
                                       ctx.data_ptr() + 4 * q_col, batch, heads, C // heads, tq, tk, int(q_strides[0]),
                                       int(q_strides[1]), int(k_strides[0]), int(k_strides[1]), _stream()), "mvq_attention_f32")
    return ctx


# ---------------------------------------------- full-sequence attention and the packet-loss fill (PLC/PLC1.py:349-422)
ATTN_SEQ_MAX_T = 8192          # PosEnc1D(max_len=8192): the reference itself fails beyond
ATTN_SEQ_BWD_MAX_T = 512


def attention_fits(dh, tq, tk) -> bool:
    """True when mvq_attention_f32 (one head slice in 64 KiB of LDS) accepts the shape."""
    return tq <= 64 and tk <= 64 and dh * (tq + 2 * tk) + tq * tk <= 16384


def attention_bwd_fits(dh, tq, tk) -> bool:
    """True when mvq_attention_bwd_f32 accepts the shape (Tq, Tk <= 32 and its LDS staging fits 64 KiB)."""
    return tq <= 32 and tk <= 32 and dh * (2 * tq + 2 * tk) + 2 * tq * tk <= 16384


def _attn_dims(q, k, folded_batch):
    B, C, Tq = q.shape
    Tk = k.shape[2]
    if folded_batch is None:
        return B, Tq, Tk, (0, 0, 0, 0)
    B = folded_batch
    if q.shape[0] != 1 or Tq % B or Tk % B:
        raise MvqError("attention: folded tensors must be [1, C, B*T]")
    Tq, Tk = Tq // B, Tk // B
    return B, Tq, Tk, (Tq, B * Tq, Tk, B * Tk)


def attention_seq(q, k, v, heads, folded_batch=None, kmask=None):
    """softmax(Q K^T / sqrt(dh)) V over whole sequences (Tq, Tk <= 8192): the arithmetic of ``attention`` -- bit-equal to it
    wherever that kernel accepts the shape -- without its 64-token limit.
    ``kmask`` (uint8 [B, Tk] on the device, nonzero = key present): mvq_attention_seq_masked_f32, item b attends over its present
    keys only, bit-equal to this call on the compacted K / V; its backward is attention_seq_bwd(kmask=)."""
    q = _dev(q, "q"); k = _dev(k, "k"); v = _dev(v, "v")
    B, Tq, Tk, strides = _attn_dims(q, k, folded_batch)
    C = q.shape[1]
    ctx = torch.empty_like(q)
    if kmask is not None:
        kmask = _key_mask_u8("attention_seq", kmask, q.device)
        if tuple(kmask.shape) != (B, Tk):
            raise MvqError(f"attention_seq: kmask {tuple(kmask.shape)} does not match [B={B}, Tk={Tk}]")
        check(_lib.lib().mvq_attention_seq_masked_f32(q.data_ptr(), k.data_ptr(), v.data_ptr(), kmask.data_ptr(), ctx.data_ptr(), B,
                                                      heads, C // heads, Tq, Tk, *strides, Tk, _stream()),
              "mvq_attention_seq_masked_f32")
        return ctx
    check(_lib.lib().mvq_attention_seq_f32(q.data_ptr(), k.data_ptr(), v.data_ptr(), ctx.data_ptr(), B, heads, C // heads,
                                           Tq, Tk, *strides, _stream()), "mvq_attention_seq_f32")
    return ctx


def attention_seq_bwd(q, k, v, g, heads, folded_batch=None, kmask=None):
    """-> (gq, gk, gv) of attention_seq for Tq, Tk <= 512.  ``kmask`` (uint8 [B, Tk], nonzero = key present):
    mvq_attention_seq_masked_bwd_f32 -- gq, and gk / gv at the present columns, are this call's on the compacted K / V bit for
    bit; gk / gv at an absent column are +0."""
    q = _dev(q, "q"); k = _dev(k, "k"); v = _dev(v, "v"); g = _dev(g, "g")
    B, Tq, Tk, strides = _attn_dims(q, k, folded_batch)
    C = q.shape[1]
    gq, gk, gv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    nbytes = _lib.lib().mvq_attention_seq_bwd_scratch_bytes(B, heads, Tq, Tk) if Tq <= ATTN_SEQ_BWD_MAX_T and Tk <= ATTN_SEQ_BWD_MAX_T else 0
    scratch = torch.empty(max(nbytes // 4, 4), device=q.device, dtype=torch.float32)
    if kmask is not None:
        kmask = _key_mask_u8("attention_seq_bwd", kmask, q.device)
        if tuple(kmask.shape) != (B, Tk):
            raise MvqError(f"attention_seq_bwd: kmask {tuple(kmask.shape)} does not match [B={B}, Tk={Tk}]")
        check(_lib.lib().mvq_attention_seq_masked_bwd_f32(q.data_ptr(), k.data_ptr(), v.data_ptr(), kmask.data_ptr(), g.data_ptr(),
                                                          gq.data_ptr(), gk.data_ptr(), gv.data_ptr(), scratch.data_ptr(), B, heads,
                                                          C // heads, Tq, Tk, *strides, Tk, _stream()),
              "mvq_attention_seq_masked_bwd_f32")
        return gq, gk, gv
    check(_lib.lib().mvq_attention_seq_bwd_f32(q.data_ptr(), k.data_ptr(), v.data_ptr(), g.data_ptr(), gq.data_ptr(),
                                               gk.data_ptr(), gv.data_ptr(), scratch.data_ptr(), B, heads, C // heads, Tq, Tk,
                                               *strides, _stream()), "mvq_attention_seq_bwd_f32")
    return gq, gk, gv


def channel_draw(ch, nb, T, packet_tok, B, stream=0, step=0, item_base=0, device=None):
    """Per-token loss pattern uint8 [B, T] of a packets.Channel on the device (mvq_channel_draw_u8): token t takes packet
    t // packet_tok; 0 = lost, otherwise the books that arrive.  Equals np.repeat(packets.channel_counts(ch, nb, P, B, stream,
    step, item_base), packet_tok, axis=1)[:, :T] bit for bit; no host read."""
    from . import packets
    if not isinstance(ch, packets.Channel):
        raise MvqError("channel_draw: ch must be a packets.Channel")
    nb, T, packet_tok, B = int(nb), int(T), int(packet_tok), int(B)
    if B < 0 or T < 0 or packet_tok < 1 or not 1 <= ch.min_books <= nb <= 255:
        raise MvqError(f"channel_draw: bad shape (B={B}, T={T}, packet_tok={packet_tok}, min_books={ch.min_books}, nb={nb})")
    out = torch.empty((B, T), device=torch.device("cuda") if device is None else device, dtype=torch.uint8)
    m = 0xFFFFFFFF
    check(_lib.lib().mvq_channel_draw_u8(out.data_ptr(), B, T, packet_tok, nb, ch.min_books, *ch.thresholds(), ch.seed & m,
                                         int(step) & m, int(stream) & m, int(item_base) & m, _stream()), "mvq_channel_draw_u8")
    return out


def hold_fill_(x, valid, carry=None, slots=None, slots_dev=None):
    """In place on contiguous fp32 x[B, C, T]: a token with valid[b, t] == 0 (valid: uint8 [B, T]) takes the values of the most
    recent valid token of its item; before the first one it takes carry[b] (``carry`` [B, C] fp32 or None = +0).  Afterwards
    carry[b] = x[b, :, T-1], so a sequence is filled piece by piece (mvq_hold_fill_f32; pure copies).  Returns x.
    ``slots`` (host integers, one per item; ``slots_dev``: their int32 device copy when the caller uploaded it already): the items
    are sessions of a pool and ``carry`` is the pool's buffer [S, C] -- item b reads and writes row slots[b] of it, every other
    row stays as it is (mvq_hold_fill_slots_f32, the same kernel body).  An out-of-range or repeated slot is refused here."""
    if not isinstance(x, torch.Tensor) or x.device.type != "cuda" or x.dtype != torch.float32 or x.dim() != 3 or not x.is_contiguous():
        raise MvqError("hold_fill_: x must be a contiguous fp32 tensor [B, C, T] on the device (it is filled in place)")
    B, C, T = x.shape
    if not isinstance(valid, torch.Tensor) or valid.device != x.device or valid.dtype != torch.uint8 or tuple(valid.shape) != (B, T) \
            or not valid.is_contiguous():
        raise MvqError(f"hold_fill_: valid must be a contiguous uint8 tensor [B={B}, T={T}] on the device of x")
    if slots is not None or slots_dev is not None:
        if slots is None:
            raise MvqError("hold_fill_: slots_dev is the device copy of slots; the host list is required")
        G, sd = _slot_list("hold_fill_", slots, carry, 2, slots_dev)
        if G != B or carry.shape[1] != C or carry.device != x.device:
            raise MvqError(f"hold_fill_: {G} slots of a pool {tuple(carry.shape)} for x [B={B}, C={C}, T={T}] on {x.device}")
        check(_lib.lib().mvq_hold_fill_slots_f32(x.data_ptr(), valid.data_ptr(), carry.data_ptr(), sd.data_ptr(), B, carry.shape[0], C, T,
                                                 _stream()), "mvq_hold_fill_slots_f32")
        return x
    if carry is not None and not (isinstance(carry, torch.Tensor) and carry.device == x.device and carry.dtype == torch.float32
                                  and tuple(carry.shape) == (B, C) and carry.is_contiguous()):
        raise MvqError(f"hold_fill_: carry must be a contiguous fp32 tensor [B={B}, C={C}] on the device of x")
    check(_lib.lib().mvq_hold_fill_f32(x.data_ptr(), valid.data_ptr(), _p(carry), B, C, T, _stream()), "mvq_hold_fill_f32")
    return x


def _mask_u8(mask, B, T, device):
    if not isinstance(mask, torch.Tensor) or mask.device != device:
        raise MvqError("plc_mask_fill: mask must be a tensor on the device of zt")
    m = mask.reshape(mask.shape[0], -1) if mask.dim() == 3 else mask            # [B,1,T] or [B,T]
    if tuple(m.shape) != (B, T):
        raise MvqError(f"plc_mask_fill: mask shape {tuple(mask.shape)} does not match [B={B}, T={T}]")
    m = m.contiguous()
    if m.dtype == torch.bool:
        return m.view(torch.uint8)                                              # 0 / 1 bytes: a view, no launch
    return m if m.dtype == torch.uint8 else (m != 0).view(torch.uint8)


def plc_mask_fill(zt, z_pred, mask, folded_batch=None, want_zt_in=True):
    """-> (zt_in, z_filled): zt_in = zt * (~mask), z_filled = where(mask, z_pred, zt_in) (PLC/PLC1.py:401-410).
    mask: bool / uint8 [B, T] or [B, 1, T] (True = token lost).  Token-folded [1,C,B*T] inputs with ``folded_batch=B``.
    ``z_pred=None`` computes zt_in alone (z_filled is None)."""
    zt = _dev(zt, "zt")
    if z_pred is not None:
        z_pred = _dev(z_pred, "z_pred")
        if z_pred.shape != zt.shape:
            raise MvqError("plc_mask_fill: z_pred must have the shape of zt")
    B, C, T, sb, sc = _fold_dims(zt, folded_batch)
    m = _mask_u8(mask, B, T, zt.device)
    zt_in = torch.empty_like(zt) if (want_zt_in or z_pred is None) else None
    zf = torch.empty_like(zt) if z_pred is not None else None
    check(_lib.lib().mvq_plc_mask_fill_f32(zt.data_ptr(), _p(z_pred), m.data_ptr(), _p(zt_in), _p(zf),
                                           B, C, T, sb, sc, _stream()), "mvq_plc_mask_fill_f32")
    return zt_in, zf


def plc_mask_fill_bwd(g, mask, folded_batch=None):
    """g_zpred = where(mask, g, 0): the gradient of z_filled w.r.t. z_pred."""
    g = _dev(g, "g")
    B, C, T, sb, sc = _fold_dims(g, folded_batch)
    m = _mask_u8(mask, B, T, g.device)
    gz = torch.empty_like(g)
    check(_lib.lib().mvq_plc_mask_fill_bwd_f32(g.data_ptr(), m.data_ptr(), gz.data_ptr(), B, C, T, sb, sc, _stream()),
          "mvq_plc_mask_fill_bwd_f32")
    return gz


# ------------------------------------------------------------ PLC evaluation (csrc/mel_ssim.hip)
MEL_SSIM_MAX_WIDTH = 32768      # frames of one image (8192 tokens = 20481 frames)
MEL_SSIM_ROWS = 64
SSIM_MODES = {"norm": 0, "ssim": 1}


def _u8_vec(mask, name):
    if not isinstance(mask, torch.Tensor) or mask.device.type != "cuda":
        raise MvqError(f"{name}: mask must be a tensor on the device")
    m = mask.reshape(-1).contiguous()
    if m.dtype == torch.bool:
        return m.view(torch.uint8)
    return m if m.dtype == torch.uint8 else (m != 0).view(torch.uint8)


def frame_subsets(latent_mask, T_wave, n_frames, hop=128, out_counts=None):
    """Token mask [T_lat] -> (frame_mask uint8 [n_frames], cols int32 [2, n_frames], counts int32 [2]): the float64
    frame -> token rule of compute_stsim_mel_with_mask and the compacted frame lists of the lost (cols[0]) and kept (cols[1])
    sides, of which the first counts[0] / counts[1] entries are valid (the counts stay on the device).  ``out_counts`` (an int32 view
    of length 2) receives the counts instead of a fresh tensor."""
    m = _u8_vec(latent_mask, "frame_subsets")
    if n_frames < 0 or n_frames > MEL_SSIM_MAX_WIDTH or T_wave < 0 or hop <= 0:
        raise MvqError(f"frame_subsets: n_frames = {n_frames} outside [0, {MEL_SSIM_MAX_WIDTH}]")
    dev = m.device
    fm = torch.empty(n_frames, device=dev, dtype=torch.uint8)
    cols = torch.empty(2, n_frames, device=dev, dtype=torch.int32)
    counts = out_counts if out_counts is not None else torch.empty(2, device=dev, dtype=torch.int32)
    if counts.dtype != torch.int32 or counts.numel() != 2 or not counts.is_contiguous() or counts.device != dev:
        raise MvqError("frame_subsets: out_counts must be a contiguous int32 [2] on the device")
    check(_lib.lib().mvq_frame_subsets(_p(m) if m.numel() else None, m.numel(), int(T_wave), int(hop), int(n_frames),
                                       _p(fm) if n_frames else None, _p(cols[0]) if n_frames else None,
                                       _p(cols[1]) if n_frames else None, counts.data_ptr(), _stream()), "mvq_frame_subsets")
    return fm, cols, counts


def mel_ssim(mel, maxv, desc, widths, max_width, cols=None, mode="ssim"):
    """Scores of N mel image pairs -> float64 [N] (one launch, csrc/mel_ssim.hip).  mel: the un-normalised [64, ld] plane;
    maxv: float32 per-item maxima (ops.mel_max); desc: int32 [N, 5] = (x column base, y column base, x max index, y max index,
    list offset or -1); widths: int32 [N] on the device, each <= max_width (a host bound); cols: int32 column lists.
    mode "ssim" (skimage's defaults; widths 1..6 fall through to the norm formula) or "norm"; width 0 gives NaN."""
    mel = _dev(mel, "mel"); maxv = _dev(maxv, "maxv")
    if mel.dim() == 3 and mel.shape[0] == 1:
        mel = mel[0]
    if mel.dim() != 2 or mel.shape[0] != MEL_SSIM_ROWS:
        raise MvqError(f"mel_ssim: the mel plane must be [{MEL_SSIM_ROWS}, ld], got {tuple(mel.shape)}")
    if mode not in SSIM_MODES:
        raise MvqError(f"mel_ssim: mode {mode!r} is not one of {sorted(SSIM_MODES)}")
    if not 0 <= int(max_width) <= min(MEL_SSIM_MAX_WIDTH, mel.shape[1]):
        raise MvqError(f"mel_ssim: max_width = {max_width} outside [0, min({MEL_SSIM_MAX_WIDTH}, ld = {mel.shape[1]})]")
    for t, name in ((desc, "desc"), (widths, "widths")) + (((cols, "cols"),) if cols is not None else ()):
        if not isinstance(t, torch.Tensor) or t.device != mel.device or t.dtype != torch.int32:
            raise MvqError(f"mel_ssim: {name} must be an int32 tensor on the device of mel")
    desc, widths = desc.contiguous(), widths.contiguous()
    n = widths.numel()
    if tuple(desc.shape) != (n, 5):
        raise MvqError(f"mel_ssim: desc must be [N = {n}, 5], got {tuple(desc.shape)}")
    cols = cols.contiguous() if cols is not None else None
    out = torch.empty(n, device=mel.device, dtype=torch.float64)
    check(_lib.lib().mvq_mel_ssim_f32(mel.data_ptr(), mel.shape[0], mel.stride(0), maxv.data_ptr(), maxv.numel(), desc.data_ptr(),
                                      _p(cols), 0 if cols is None else cols.numel(), widths.data_ptr(), n, int(max_width),
                                      SSIM_MODES[mode], out.data_ptr(), _stream()), "mvq_mel_ssim_f32")
    return out


def subset_stats(ref, est, latent_mask):
    """-> float64 [8]: per side (lost, kept) the count, sum |r-e|, sum r^2, sum (r-e)^2 of ref / est [T] under the float32
    sample -> token rule of token_to_sample_mask (one launch)."""
    ref = _dev(ref, "ref").reshape(-1); est = _dev(est, "est").reshape(-1)
    if ref.numel() != est.numel():
        raise MvqError("subset_stats: ref and est must have the same length")
    m = _u8_vec(latent_mask, "subset_stats")
    out = torch.empty(8, device=ref.device, dtype=torch.float64)
    check(_lib.lib().mvq_subset_stats_f32(ref.data_ptr(), est.data_ptr(), ref.numel(), _p(m) if m.numel() else None, m.numel(),
                                          out.data_ptr(), _stream()), "mvq_subset_stats_f32")
    return out


_AR_CHECKED = set()


def ar_latents_fused(zt, z_run, *, k_all, v_all, t_audio, pe, ln_q, wq, wo, ln_f, w1, b1, w3, b3, ln_eps, tok, tok_eps, scale,
                     wd, bd, wu, bu, books, books_use, heads, c_ff, code_dim, r_tokens=None, idx_out=None, tactile_only=False, chunk=16,
                     staged=False, z_prev=None, z_last_out=None, rate=None, beam=1):
    """The whole chunked AR loop as ONE persistent kernel (csrc/ar_fused.hip: mvq_ar_latents_f32): zt[B,C,Tlat] -> z_run[B,C,Tlat]
    (written in place), optionally r_tokens[B,96,Tlat] and idx_out[nb,B,Tlat] (int32).  ``k_all`` / ``v_all``: token-folded K / V
    of all chunks ([1,C,B*t_audio], CrossPredictor.keys_values) or None; the w* are K-major packed 1x1 weights (pack_conv1d);
    ln_q / ln_f / tok = (weight, bias).  ``staged``: the same stages as stand-alone launches issued by ONE host call
    (mvq_ar_latents_staged_f32; batch <= 8) instead of the persistent kernel.  Same bits as the Python loop either way
    (tests/test_gpu_ar_fused.py).  ``z_prev`` / ``z_last_out`` ([B, C] fp32, staged only): the token carried into and out of a
    piece of a longer sequence (mvq_ar_latents_staged_carry_f32).  ``rate`` (staged only) = (packet_tok, min_books, mode, tol2,
    budget, nb_valid_out uint8 [B, Tlat], nb_sent_out uint8 [B, P]): closed-loop rate control, one mvq_rvq_rate_f32 launch per chunk
    (mvq_ar_latents_staged_rate_f32); needs idx_out.  ``beam`` > 1 (with ``rate``): each chunk's search is the beam search
    (mvq_ar_latents_staged_rate_beam_f32); 1 is the call above, the new export is not touched."""
    carried = z_prev is not None or z_last_out is not None
    if int(beam) != 1 and rate is None:
        raise MvqError("ar_latents_fused: beam needs rate (the closed loop forms the receiver's sum from the beam's indices)")
    if rate is not None and (not staged or idx_out is None):
        raise MvqError("ar_latents_fused: rate needs staged=True and idx_out (the persistent kernel has no rate stage)")
    if carried and not staged:
        raise MvqError("ar_latents_fused: z_prev / z_last_out need staged=True (the persistent kernel carries no token)")
    zt = _dev(zt, "zt")
    B, C, Tl = zt.shape
    nb_all, K = (books.shape[0], books.shape[1]) if books is not None else (0, 1)
    nb = nb_all if books_use is None else max(0, min(int(books_use), nb_all))
    a = _lib.ArArgs()
    a.batch, a.t_lat, a.t_audio, a.tactile_only, a.books_use, a.rvq_k = B, Tl, int(t_audio), int(bool(tactile_only)), nb, K
    a.c_lat, a.c_ff, a.code_dim, a.heads, a.chunk = C, int(c_ff), int(code_dim), int(heads), int(chunk)
    a.ln_eps, a.tok_eps, a.scale = float(ln_eps), float(tok_eps), float(scale)
    a.zt, a.z_run, a.r_tokens, a.idx_out = zt.data_ptr(), z_run.data_ptr(), _p(r_tokens), _p(idx_out)
    a.k_all, a.v_all, a.pe = _p(k_all), _p(v_all), _p(pe)
    (a.lnq_g, a.lnq_b), (a.lnf_g, a.lnf_b), (a.tok_g, a.tok_b) = map(lambda t: (_p(t[0]), _p(t[1])), (ln_q, ln_f, tok))
    a.wq, a.wo, a.w1, a.b1, a.w3, a.b3 = _p(wq), _p(wo), _p(w1), _p(b1), _p(w3), _p(b3)
    a.wd, a.bd, a.wu, a.bu, a.books = _p(wd), _p(bd), _p(wu), _p(bu), _p(books)
    L = _lib.lib()
    nbytes = L.mvq_ar_workspace_bytes(B, Tl)
    ws = torch.empty(max(nbytes, 4), device=zt.device, dtype=torch.uint8)
    if rate is not None:
        packet_tok, min_books, mode, tol2, budget, nbv, nbs = rate
        if int(beam) != 1:
            check(L.mvq_ar_latents_staged_rate_beam_f32(ctypes.byref(a), int(packet_tok), int(min_books), int(mode), float(tol2), int(budget),
                                                        int(beam), _p(z_prev), _p(z_last_out), nbv.data_ptr(), nbs.data_ptr(), ws.data_ptr(),
                                                        nbytes, _stream()), "mvq_ar_latents_staged_rate_beam_f32")
            return z_run
        check(L.mvq_ar_latents_staged_rate_f32(ctypes.byref(a), int(packet_tok), int(min_books), int(mode), float(tol2), int(budget),
                                               _p(z_prev), _p(z_last_out), nbv.data_ptr(), nbs.data_ptr(), ws.data_ptr(), nbytes,
                                               _stream()), "mvq_ar_latents_staged_rate_f32")
        return z_run
    if carried:
        check(L.mvq_ar_latents_staged_carry_f32(ctypes.byref(a), _p(z_prev), _p(z_last_out), ws.data_ptr(), nbytes, _stream()),
              "mvq_ar_latents_staged_carry_f32")
        return z_run
    if staged:
        check(L.mvq_ar_latents_staged_f32(ctypes.byref(a), ws.data_ptr(), nbytes, _stream()), "mvq_ar_latents_staged_f32")
        return z_run
    check(L.mvq_ar_latents_f32(ctypes.byref(a), ws.data_ptr(), nbytes, _stream()), "mvq_ar_latents_f32")
    key = (B, Tl, zt.device.index, bool(tactile_only))
    if key not in _AR_CHECKED:            # co-residency of the persistent grid is a property of the shape: verified on its first use
        check(L.mvq_ar_check(ws.data_ptr(), _stream()), "mvq_ar_check")
        _AR_CHECKED.add(key)
    return z_run


def gelu(x):
    x = _dev(x, "x")
    y = torch.empty_like(x)
    check(_lib.lib().mvq_gelu_f32(x.data_ptr(), y.data_ptr(), x.numel(), _stream()), "mvq_gelu_f32")
    return y


def fold_time_slice(a, s, e):
    """a[B,C,T][..., s:e] -> token-folded [1, C, B*(e-s)] (column b*(e-s)+i = token i of batch element b)."""
    a = _dev(a, "a")
    B, C, T = a.shape
    n = e - s
    y = torch.empty(1, C, B * n, device=a.device, dtype=torch.float32)
    check(_lib.lib().mvq_copy3d_f32(a.data_ptr() + 4 * s, C * T, T, y.data_ptr(), n, B * n, B, C, n, _stream()),
          "mvq_copy3d_f32")
    return y


def unfold_into_(dst, s, src, batch):
    """dst[B,C,T][..., s:s+n] = unfold(src[1, C, B*n])."""
    B, C, T = dst.shape
    n = src.shape[2] // batch
    check(_lib.lib().mvq_copy3d_f32(src.data_ptr(), n, B * n, dst.data_ptr() + 4 * s, C * T, T, B, C, n, _stream()),
          "mvq_copy3d_f32")
    return dst


def fold_column_into_(dst_folded, col, src, t, batch):
    """dst_folded[1,C,B*n][:, :, b*n + col] = src[B,C,T][b, :, t]."""
    B, C, T = src.shape
    n = dst_folded.shape[2] // batch
    check(_lib.lib().mvq_copy3d_f32(src.data_ptr() + 4 * t, C * T, T, dst_folded.data_ptr() + 4 * col, n, B * n,
                                    B, C, 1, _stream()), "mvq_copy3d_f32")
    return dst_folded


def copy_strided_(dst, dst_col, dst_strides, src, src_col, src_strides, batch, c, n):
    """dst[dst_col + b*ds0 + ch*ds1 + i] = src[src_col + b*ss0 + ch*ss1 + i] for b < batch, ch < c, i < n (flat fp32 offsets;
    a zero stride repeats).  Bounds are checked against both tensors."""
    for t, col, (s0, s1) in ((dst, dst_col, dst_strides), (src, src_col, src_strides)):
        if batch and c and n and col + (batch - 1) * s0 + (c - 1) * s1 + n > t.numel():
            raise MvqError("copy_strided_: the copy reaches past the end of a tensor")
    check(_lib.lib().mvq_copy3d_f32(src.data_ptr() + 4 * src_col, int(src_strides[0]), int(src_strides[1]),
                                    dst.data_ptr() + 4 * dst_col, int(dst_strides[0]), int(dst_strides[1]), batch, c, n, _stream()),
          "mvq_copy3d_f32")
    return dst


def sub(a, b):
    """a - b for equal-shaped contiguous tensors."""
    a = _dev(a, "a"); b = _dev(b, "b")
    y = torch.empty_like(a)
    n = a.numel()
    check(_lib.lib().mvq_sub3d_f32(a.data_ptr(), 0, 0, b.data_ptr(), 0, 0, y.data_ptr(), 0, 0, 1, 1, n, _stream()),
          "mvq_sub3d_f32")
    return y


def align_xcorr(ref, est, max_shift=200):
    """Correlations c(s), s in [-max_shift, max_shift], of equal-length 1-D signals and the best shift (device int32)."""
    ref = _dev(ref, "ref").reshape(-1); est = _dev(est, "est").reshape(-1)
    if ref.numel() != est.numel():
        raise MvqError("align_xcorr: crop_match the signals first (equal lengths)")
    n = 2 * max_shift + 1
    corr = torch.empty(n, device=ref.device, dtype=torch.float32)
    scratch = torch.empty(n, device=ref.device, dtype=torch.int32)
    best = torch.zeros(1, device=ref.device, dtype=torch.int32)
    check(_lib.lib().mvq_align_xcorr_f32(ref.data_ptr(), est.data_ptr(), ref.numel(), max_shift, corr.data_ptr(),
                                         scratch.data_ptr(), best.data_ptr(), _stream()), "mvq_align_xcorr_f32")
    return corr, best


def align_xcorr_batch(ref, est, max_shift=200):
    """Best shift per item for ref[B,T] / est[B,T] (equal lengths): ONE launch pair for the whole batch (grid dimension =
    item), NO host sync; returns the int32 device tensor of shifts."""
    ref = _dev(ref, "ref"); est = _dev(est, "est")
    if ref.shape != est.shape or ref.dim() != 2:
        raise MvqError("align_xcorr_batch: ref and est must both be [B, T]")
    B, T = ref.shape
    n = 2 * max_shift + 1
    corr = torch.empty(B, n, device=ref.device, dtype=torch.float32)
    scratch = torch.empty(B, n, device=ref.device, dtype=torch.int32)
    best = torch.zeros(B, device=ref.device, dtype=torch.int32)
    check(_lib.lib().mvq_align_xcorr_batch_f32(ref.data_ptr(), est.data_ptr(), B, T, max_shift, corr.data_ptr(),
                                               scratch.data_ptr(), best.data_ptr(), _stream()), "mvq_align_xcorr_batch_f32")
    return best


def resample_ragged(x, kern, off, length, orig, newf, width, lout_pitch):
    """Rows x[b, off[b] : off[b] + length[b]] resampled by the filter bank kern[newf, 2*width + orig] in one launch.
    off / length: int32 device tensors [B].  -> (y[B, lout_pitch] zero past each row's output length, lout int32 [B])."""
    x = _dev(x, "x")
    if x.dim() != 2 or off.dtype != torch.int32 or length.dtype != torch.int32 or not off.is_cuda or not length.is_cuda:
        raise MvqError("resample_ragged: x must be [B, L]; off / length int32 HIP tensors")
    B, L = x.shape
    y = torch.empty(B, lout_pitch, device=x.device, dtype=torch.float32)
    lout = torch.empty(B, device=x.device, dtype=torch.int32)
    check(_lib.lib().mvq_resample_ragged_f32(x.data_ptr(), kern.data_ptr(), y.data_ptr(), off.data_ptr(), length.data_ptr(),
                                             lout.data_ptr(), B, L, lout_pitch, orig, newf, width, kern.shape[1], _stream()),
          "mvq_resample_ragged_f32")
    return y, lout


def resample_stream_state(orig, width, batch, device):
    """A new session's state for resample_stream: zeros [batch, ceil(width/orig)*orig + width] (layout: include/mvq.h)."""
    hold = (int(width) + int(orig) - 1) // int(orig)
    return torch.zeros(int(batch), hold * int(orig) + int(width), device=device, dtype=torch.float32)


def _resample_stream(who, x_new, kern, state, sd, consumed, orig, newf, width, final):
    """resample_stream and resample_stream_slots: ``sd`` None for the dense sessions state[B, S], else the group's device slot
    list (_slot_list has checked ``state`` then)."""
    x_new = _dev(x_new, "x_new")
    if state.dim() != 2 or state.dtype != torch.float32 or not state.is_cuda or not state.is_contiguous() or x_new.dim() != 2 \
            or x_new.shape[0] != (state.shape[0] if sd is None else sd.shape[0]) or x_new.device != state.device:
        raise MvqError(f"{who}: x_new must be [B, n_new], one row per session, on the device of state, a contiguous fp32 HIP tensor "
                       f"[sessions, S]; got {tuple(x_new.shape)} and {tuple(state.shape)}")
    B, n_new = x_new.shape
    consumed, orig, newf, width = int(consumed), int(orig), int(newf), int(width)
    if orig <= 0 or width < 0 or state.shape[1] != (width + orig - 1) // orig * orig + width:
        raise MvqError(f"{who}: state {tuple(state.shape)} does not fit orig={orig}, width={width}")
    if not final and n_new % orig:
        raise MvqError(f"{who}: a piece of {n_new} samples is no multiple of {orig}; only the final one may be")
    n_out = resample_stream_out_len(consumed, n_new, orig, width, final)
    y = torch.empty(B, n_out, device=x_new.device, dtype=torch.float32)
    tail = (n_new, consumed, int(bool(final)), n_out, orig, newf, width, kern.shape[1], _stream())
    if sd is None:
        check(_lib.lib().mvq_resample_stream_f32(x_new.data_ptr(), kern.data_ptr(), state.data_ptr(), y.data_ptr(), B, *tail),
              "mvq_resample_stream_f32")
    else:
        check(_lib.lib().mvq_resample_stream_slots_f32(x_new.data_ptr(), kern.data_ptr(), state.data_ptr(), sd.data_ptr(), B,
                                                       state.shape[0], y.data_ptr(), *tail), "mvq_resample_stream_slots_f32")
    return y


def resample_stream(x_new, kern, state, consumed, orig, newf, width, final=False):
    """The next piece x_new[B, n_new] of a decimated stream -> the outputs y[B, n_out] it completes (mvq_resample_stream_f32);
    ``state`` (resample_stream_state) is updated in place, ``consumed`` = samples given to earlier calls."""
    return _resample_stream("resample_stream", x_new, kern, state, None, consumed, orig, newf, width, final)


def _stream_window(who, hist, h_in, z_new, h_out, sd):
    """stream_window and stream_window_slots: ``sd`` None for the dense sessions hist[B, C, cap], else the group's device slot
    list."""
    z_new = _dev(z_new, "z_new")
    if not isinstance(hist, torch.Tensor) or hist.dim() != 3 or z_new.dim() != 3 or hist.dtype != torch.float32 or not hist.is_cuda \
            or not hist.is_contiguous() or hist.device != z_new.device \
            or tuple(z_new.shape[:2]) != (hist.shape[0] if sd is None else sd.shape[0], hist.shape[1]):
        raise MvqError(f"{who}: hist must be a contiguous fp32 HIP tensor [sessions, C, cap] and z_new [B, C, n] on its device, one "
                       "block of C rows per session")
    S, C, cap = hist.shape
    B, _, n = z_new.shape
    h_in, h_out = int(h_in), int(h_out)
    win = torch.empty(B, C, max(h_in, 0) + n, device=z_new.device, dtype=torch.float32)
    if sd is None:
        check(_lib.lib().mvq_stream_window_f32(hist.data_ptr(), h_in, z_new.data_ptr(), n, win.data_ptr(), h_out, cap, B, C, _stream()),
              "mvq_stream_window_f32")
    else:
        check(_lib.lib().mvq_stream_window_slots_f32(hist.data_ptr(), sd.data_ptr(), B, S, h_in, z_new.data_ptr(), n, win.data_ptr(),
                                                     h_out, cap, C, _stream()), "mvq_stream_window_slots_f32")
    return win


def stream_window(hist, h_in, z_new, h_out):
    """win[B, C, h_in + n] = [hist[..., :h_in] | z_new[B, C, n]], then hist[..., :h_out] <- the last h_out columns of win, in one
    launch (mvq_stream_window_f32).  hist: contiguous fp32 [B, C, cap], updated in place."""
    return _stream_window("stream_window", hist, h_in, z_new, h_out, None)


# ---------------------------------------------------------------------------------- receiver pool
def _slot_host(who, slots, pool, dims, dtype=torch.float32):
    """The slot rule of every pool call: ``slots`` as HOST integers, refused here, before anything else is looked at, when one is
    out of range or repeated, so no unchecked index reaches the device.  -> the list.  ``pool``: the state buffer, [n_slots, ...]
    of ``dims`` dimensions."""
    if not isinstance(pool, torch.Tensor) or pool.dim() != dims:
        raise MvqError(f"{who}: the pool buffer must be a tensor of {dims} dimensions")
    try:
        if isinstance(slots, torch.Tensor):
            raise TypeError
        host = [operator.index(v) for v in slots]
    except TypeError:
        raise MvqError(f"{who}: slots must be a sequence of host integers") from None
    n_slots = pool.shape[0]
    bad = [v for v in host if not 0 <= v < n_slots]
    if bad:
        raise MvqError(f"{who}: slot {bad[0]} outside the pool's [0, {n_slots})")
    if len(set(host)) != len(host):
        raise MvqError(f"{who}: a slot is listed twice in {host} (two blocks would update one row)")
    if pool.dtype != dtype or not pool.is_cuda or not pool.is_contiguous():
        raise MvqError(f"{who}: the pool buffer must be a contiguous {'fp32' if dtype == torch.float32 else dtype} HIP tensor")
    return host


def _slot_list(who, slots, pool, dims, slots_dev, dtype=torch.float32):
    """_slot_host -> (G, int32 device tensor [G]); ``slots_dev`` is that tensor when the caller uploaded the list already
    (StreamReceiverPool sends the lists of a whole tick with its packet bodies), else it is uploaded here."""
    host = _slot_host(who, slots, pool, dims, dtype)
    if slots_dev is None:
        slots_dev = torch.tensor(host, dtype=torch.int32).to(pool.device)
    elif not isinstance(slots_dev, torch.Tensor) or slots_dev.dtype != torch.int32 or slots_dev.device != pool.device \
            or tuple(slots_dev.shape) != (len(host),) or not slots_dev.is_contiguous():
        raise MvqError(f"{who}: slots_dev must be the contiguous int32 tensor [{len(host)}] of the list on {pool.device}")
    return len(host), slots_dev


def stream_rows(pool, slots, rows=None, slots_dev=None):
    """The carried token of a group (mvq_stream_rows_f32).  ``rows`` None: gather, -> rows[G, C] = pool[slots]; ``rows`` [G, C]:
    scatter, pool[slots] = rows (-> pool).  pool: contiguous fp32 [S, C] on the device, ``slots`` host integers."""
    G, sd = _slot_list("stream_rows", slots, pool, 2, slots_dev)
    S, C = pool.shape
    scatter = rows is not None
    if scatter:
        if not isinstance(rows, torch.Tensor) or rows.dtype != torch.float32 or not rows.is_contiguous() \
                or tuple(rows.shape) != (G, C) or rows.device != pool.device:
            raise MvqError(f"stream_rows: rows must be a contiguous fp32 tensor [G={G}, C={C}] on the pool's device")
    else:
        rows = torch.empty(G, C, device=pool.device, dtype=torch.float32)
    check(_lib.lib().mvq_stream_rows_f32(pool.data_ptr(), sd.data_ptr(), G, S, rows.data_ptr(), C, int(scatter), _stream()),
          "mvq_stream_rows_f32")
    return pool if scatter else rows


AUDIO_FADE_STATE = 11       # stream.DEC_HALO_TOK + 1 run lengths per session (include/mvq.h, mvq_audio_fade_f32)


def audio_fade_state(rows, device):
    """A fade state for ``rows`` sessions: zeros int32 [rows, 11] -- "no loss so far" (layout: include/mvq.h).  A session's first
    step does not read its row, so a pool never has to clear one."""
    return torch.zeros(int(rows), AUDIO_FADE_STATE, device=device, dtype=torch.int32)


def audio_fade_(y, valid, state, fade, tok0, slots=None, slots_dev=None):
    """packets.AudioFade in place on a piece y[G, 1, len] (contiguous fp32 on the device) that starts at sample 320*tok0 of its item,
    for the step that brings ``valid`` (uint8 [G, n], nonzero = some stage of the token arrived; None: a finish without new
    tokens); ``state`` (audio_fade_state) moves on in place (mvq_audio_fade_f32, one launch, no host read).  The piece is what a
    streaming step emits: 320*(n - 10) + 320*min(tokens before, 10) samples for a push, everything up to 320*T - 8 for a finish;
    the whole item is tok0 = 0 with all T tokens and a scratch state row.  Returns y.
    ``slots`` (host integers, one per item; ``slots_dev`` their int32 device copy): the items are sessions of a pool and ``state`` is
    the pool's [S, 11]; an out-of-range or repeated slot is refused here (mvq_audio_fade_slots_f32, the same kernel body)."""
    from .packets import AudioFade
    if not isinstance(fade, AudioFade):
        raise MvqError("audio_fade_: fade must be a packets.AudioFade")
    if not isinstance(y, torch.Tensor) or y.device.type != "cuda" or y.dtype != torch.float32 or y.dim() != 3 or y.shape[1] != 1 \
            or not y.is_contiguous():
        raise MvqError("audio_fade_: y must be a contiguous fp32 tensor [G, 1, len] on the device (it is faded in place)")
    G, _, n_len = y.shape
    n = 0
    if valid is not None:
        if not isinstance(valid, torch.Tensor) or valid.device != y.device or valid.dtype != torch.uint8 or valid.dim() != 2 \
                or valid.shape[0] != G or not valid.is_contiguous():
            raise MvqError(f"audio_fade_: valid must be a contiguous uint8 tensor [G={G}, n] on the device of y")
        n = valid.shape[1]
    if not isinstance(state, torch.Tensor) or state.dtype != torch.int32 or state.dim() != 2 or state.shape[1] != AUDIO_FADE_STATE \
            or state.device != y.device or not state.is_contiguous():
        raise MvqError(f"audio_fade_: state must be a contiguous int32 tensor [sessions, {AUDIO_FADE_STATE}] on the device of y "
                       "(ops.audio_fade_state)")
    tail = (n, int(tok0), n_len, int(fade.hold_tok), int(fade.fade_tok), _stream())
    if slots is not None or slots_dev is not None:
        if slots is None:
            raise MvqError("audio_fade_: slots_dev is the device copy of slots; the host list is required")
        n_list, slots_dev = _slot_list("audio_fade_", slots, state, 2, slots_dev, dtype=torch.int32)
        if n_list != G:
            raise MvqError(f"audio_fade_: {n_list} slots for a piece of {G} items")
        check(_lib.lib().mvq_audio_fade_slots_f32(_p(y) if n_len else None, _p(valid) if n else None, state.data_ptr(), slots_dev.data_ptr(),
                                                  G, state.shape[0], *tail), "mvq_audio_fade_slots_f32")
        return y
    if state.shape[0] != G:
        raise MvqError(f"audio_fade_: a state of {state.shape[0]} sessions for a piece of {G} items")
    check(_lib.lib().mvq_audio_fade_f32(_p(y) if n_len else None, _p(valid) if n else None, state.data_ptr(), G, *tail), "mvq_audio_fade_f32")
    return y


def stream_window_slots(hist, slots, h_in, z_new, h_out, slots_dev=None):
    """stream_window for the sessions ``slots`` (host integers) of a pool: win[G, C, h_in + n] = [hist[slots][..., :h_in] | z_new],
    then hist[slots][..., :h_out] <- the last h_out columns of win, in one launch (mvq_stream_window_slots_f32).  hist: contiguous
    fp32 [S, C, cap], updated in place in the listed slots only."""
    _, sd = _slot_list("stream_window_slots", slots, hist, 3, slots_dev)
    return _stream_window("stream_window_slots", hist, h_in, z_new, h_out, sd)


def _stream_stage_window(who, tail, h_in, src, src_off, n, h_out, cap, tail_off, win_t, sd):
    """stream_stage_window and stream_stage_window_slots: ``sd`` None for the dense sessions, else the group's device slot list."""
    src = _dev(src, "src")
    if not isinstance(tail, torch.Tensor) or tail.dim() != 2 or src.dim() != 3 or tail.dtype != torch.float32 or not tail.is_cuda \
            or not tail.is_contiguous() or tail.device != src.device:
        raise MvqError(f"{who}: the state must be a contiguous fp32 HIP tensor [sessions, floats] and src [B, C, src_t] on its device")
    rows, stride = tail.shape
    B, C, src_t = src.shape
    h_in, src_off, n, h_out, cap, tail_off = (int(v) for v in (h_in, src_off, n, h_out, cap, tail_off))
    if sd is None and B > rows:
        raise MvqError(f"{who}: {B} sessions, the state has {rows} rows")
    if cap < 0 or tail_off < 0 or tail_off + C * cap > stride:
        raise MvqError(f"{who}: a [{C}, {cap}] tail at offset {tail_off} does not fit a state row of {stride} floats")
    win_t = max(h_in, 0) + max(n, 0) if win_t is None else int(win_t)
    win = torch.empty(B, C, max(win_t, 0), device=src.device, dtype=torch.float32)
    tp = tail.data_ptr() + 4 * tail_off
    if sd is None:
        check(_lib.lib().mvq_stream_stage_window_f32(tp, stride, h_in, src.data_ptr(), src_t, 1, src_off, n, win.data_ptr(), win_t, 1, h_out, cap,
                                                     B, C, _stream()), "mvq_stream_stage_window_f32")
    else:
        check(_lib.lib().mvq_stream_stage_window_slots_f32(tp, stride, sd.data_ptr(), B, rows, h_in, src.data_ptr(), src_t, 1, src_off, n,
                                                           win.data_ptr(), win_t, 1, h_out, cap, C, _stream()),
              "mvq_stream_stage_window_slots_f32")
    return win


def stream_stage_window(state, h_in, src, src_off, n, h_out, cap, tail_off=0, win_t=None):
    """One stage window of the stateful streaming decoder (mvq_stream_stage_window_f32): win[B, C, win_t] = [tail[..., :h_in] |
    src[..., src_off:src_off + n] | zeros], then tail[..., :h_out] <- the last h_out columns of [tail | new], in one launch.
    ``state``: contiguous fp32 [sessions, floats], updated in place; the stage's tail of session b is the [C, cap] block at
    state[b, tail_off:].  Dense rows (the packed-row forms of the entry point are the stack call's own).  ``win_t`` None: h_in + n.  With h_in + n = 0 nothing is launched and ``win`` is not written."""
    return _stream_stage_window("stream_stage_window", state, h_in, src, src_off, n, h_out, cap, tail_off, win_t, None)


def stream_stage_window_slots(state, slots, h_in, src, src_off, n, h_out, cap, tail_off=0, win_t=None, slots_dev=None):
    """stream_stage_window for the sessions ``slots`` (host integers) of a pool: session g of src / win on state[slots[g]]
    (mvq_stream_stage_window_slots_f32); unlisted rows are not touched."""
    _, sd = _slot_list("stream_stage_window_slots", slots, state, 2, slots_dev)
    return _stream_stage_window("stream_stage_window_slots", state, h_in, src, src_off, n, h_out, cap, tail_off, win_t, sd)


def stream_stage_window_snake(state, h_in, src, src_off, n, h_out, cap, alpha, tail_off=0, win_t=None, slots=None, slots_dev=None):
    """stream_stage_window with the window's Snake beside it (mvq_stream_stage_window_snake_f32 / _slots_f32; the stateful
    encoder's wide blocks) -> (win, win_s), win_s = snake(win, alpha) on the h_in + n window columns and +0
    in the zero tail; the tail stays raw.  ``alpha`` fp32 [C] (any shape of C elements).  ``slots`` None: dense sessions."""
    who = "stream_stage_window_snake"
    src = _dev(src, "src")
    alpha = _dev(alpha, "alpha").reshape(-1).contiguous()
    if not isinstance(state, torch.Tensor) or state.dim() != 2 or src.dim() != 3 or state.dtype != torch.float32 or not state.is_cuda \
            or not state.is_contiguous() or state.device != src.device:
        raise MvqError(f"{who}: the state must be a contiguous fp32 HIP tensor [sessions, floats] and src [B, C, src_t] on its device")
    rows, stride = state.shape
    B, C, src_t = src.shape
    h_in, src_off, n, h_out, cap, tail_off = (int(v) for v in (h_in, src_off, n, h_out, cap, tail_off))
    sd = None
    if slots is not None:
        _, sd = _slot_list(who, slots, state, 2, slots_dev)
    elif B > rows:
        raise MvqError(f"{who}: {B} sessions, the state has {rows} rows")
    if alpha.numel() != C or alpha.dtype != torch.float32:
        raise MvqError(f"{who}: alpha must hold {C} fp32 values")
    if cap < 0 or tail_off < 0 or tail_off + C * cap > stride:
        raise MvqError(f"{who}: a [{C}, {cap}] tail at offset {tail_off} does not fit a state row of {stride} floats")
    win_t = max(h_in, 0) + max(n, 0) if win_t is None else int(win_t)
    win = torch.empty(B, C, max(win_t, 0), device=src.device, dtype=torch.float32)
    win_s = torch.empty_like(win)
    tp = state.data_ptr() + 4 * tail_off
    if sd is None:
        check(_lib.lib().mvq_stream_stage_window_snake_f32(tp, stride, h_in, src.data_ptr(), src_t, src_off, n, win.data_ptr(), win_s.data_ptr(),
                                                           alpha.data_ptr(), win_t, h_out, cap, B, C, _stream()),
              "mvq_stream_stage_window_snake_f32")
    else:
        check(_lib.lib().mvq_stream_stage_window_snake_slots_f32(tp, stride, sd.data_ptr(), B, rows, h_in, src.data_ptr(), src_t, src_off, n,
                                                                 win.data_ptr(), win_s.data_ptr(), alpha.data_ptr(), win_t, h_out, cap, C,
                                                                 _stream()), "mvq_stream_stage_window_snake_slots_f32")
    return win, win_s


def resample_stream_slots(x_new, kern, state, slots, consumed, orig, newf, width, final=False, slots_dev=None):
    """resample_stream for the sessions ``slots`` (host integers) of a pool: x_new[G, n_new] -> y[G, n_out], state[slots] moved on
    in place (mvq_resample_stream_slots_f32).  ``consumed`` is the group's launch class -- 0, or any multiple of ``orig`` of at
    least the state's length that one member has consumed (include/mvq.h)."""
    _, sd = _slot_list("resample_stream_slots", slots, state, 2, slots_dev)
    return _resample_stream("resample_stream_slots", x_new, kern, state, sd, consumed, orig, newf, width, final)


def _rational_hold(orig, width, hold):
    return (int(width) + int(orig) - 1) // int(orig) if hold is None else int(hold)


def resample_stream_rational_state(orig, width, batch, device, hold=None):
    """A new session's state for resample_stream_rational: zeros [batch, hold*orig + width], ``hold`` (None: ceil(width/orig)) the
    lag in filter blocks (layout: include/mvq.h)."""
    return torch.zeros(int(batch), _rational_hold(orig, width, hold) * int(orig) + int(width), device=device, dtype=torch.float32)


RESAMPLE_FORMS = {"block": "", "split": "_split"}                   # form -> the infix of the entry point's name


def _resample_stream_rational(who, x_new, kern, state, sd, consumed, orig, newf, width, hold, final, form="block"):
    """resample_stream_rational and resample_stream_rational_slots: ``sd`` None for the dense sessions state[B, S], else the
    group's device slot list (_slot_list has checked ``state`` then).  The checks of _resample_stream, and the bank's.  ``form``:
    "block" = one block per session (mvq_resample_stream_rational[_slots]_f32), "split" = the two-launch form of the same call
    (mvq_resample_stream_rational_split[_slots]_f32)."""
    if form not in RESAMPLE_FORMS:
        raise MvqError(f"{who}: form must be 'block' or 'split', not {form!r}")
    x_new = _dev(x_new, "x_new")
    if state.dim() != 2 or state.dtype != torch.float32 or not state.is_cuda or not state.is_contiguous() or x_new.dim() != 2 \
            or x_new.shape[0] != (state.shape[0] if sd is None else sd.shape[0]) or x_new.device != state.device:
        raise MvqError(f"{who}: x_new must be [B, n_new], one row per session, on the device of state, a contiguous fp32 HIP tensor "
                       f"[sessions, S]; got {tuple(x_new.shape)} and {tuple(state.shape)}")
    B, n_new = x_new.shape
    consumed, orig, newf, width = int(consumed), int(orig), int(newf), int(width)
    if orig <= 0 or newf <= 0 or width < 0:
        raise MvqError(f"{who}: orig={orig}, newf={newf}, width={width}")
    hold = _rational_hold(orig, width, hold)
    if hold < (width + orig - 1) // orig or state.shape[1] != hold * orig + width:
        raise MvqError(f"{who}: state {tuple(state.shape)} does not fit orig={orig}, width={width}, hold={hold} "
                       f"(hold >= {(width + orig - 1) // orig})")
    if not isinstance(kern, torch.Tensor) or kern.dtype != torch.float32 or not kern.is_contiguous() or kern.device != state.device \
            or tuple(kern.shape) != (newf, 2 * width + orig):
        raise MvqError(f"{who}: kern must be the contiguous fp32 bank [{newf}, {2 * width + orig}] on the device of state")
    if consumed < 0 or consumed % orig:
        raise MvqError(f"{who}: consumed = {consumed} is no multiple of {orig}")
    if not final and n_new % orig:
        raise MvqError(f"{who}: a piece of {n_new} samples is no multiple of {orig}; only the final one may be")
    n_out = resample_stream_rational_out_len(consumed, n_new, orig, newf, width, hold, final)
    y = torch.empty(B, n_out, device=x_new.device, dtype=torch.float32)
    tail = (n_new, consumed, int(bool(final)), n_out, orig, newf, width, kern.shape[1], hold, _stream())
    name = f"mvq_resample_stream_rational{RESAMPLE_FORMS[form]}{'' if sd is None else '_slots'}_f32"
    fn = getattr(_lib.lib(), name)
    if sd is None:
        check(fn(x_new.data_ptr(), kern.data_ptr(), state.data_ptr(), y.data_ptr(), B, *tail), name)
    else:
        check(fn(x_new.data_ptr(), kern.data_ptr(), state.data_ptr(), sd.data_ptr(), B, state.shape[0], y.data_ptr(), *tail), name)
    return y


def resample_stream_rational(x_new, kern, state, consumed, orig, newf, width, hold=None, final=False, form="block"):
    """The next piece x_new[B, n_new] of a stream resampled by orig : newf -> the outputs y[B, n_out] it completes
    (mvq_resample_stream_rational_f32; stream.resample_stream_rational_out_len counts them).  ``kern`` [newf, 2*width + orig] is
    resample.sinc_resample_kernel's bank, ``state`` (resample_stream_rational_state) is updated in place, ``consumed`` = samples
    given to earlier calls, ``hold`` the lag in filter blocks the state was made for.  ``form="split"``: the same outputs and state
    from the two-launch form, a session's outputs spread over many blocks (the form for few sessions)."""
    return _resample_stream_rational("resample_stream_rational", x_new, kern, state, None, consumed, orig, newf, width, hold, final, form)


def resample_stream_rational_slots(x_new, kern, state, slots, consumed, orig, newf, width, hold=None, final=False, slots_dev=None,
                                   form="block"):
    """resample_stream_rational for the sessions ``slots`` (host integers) of a pool: x_new[G, n_new] -> y[G, n_out], state[slots]
    moved on in place (mvq_resample_stream_rational_slots_f32).  ``consumed`` is the group's launch class -- 0, or any multiple of
    ``orig`` of at least the state's length that one member has consumed (include/mvq.h).  ``form``: resample_stream_rational's."""
    _, sd = _slot_list("resample_stream_rational_slots", slots, state, 2, slots_dev)
    return _resample_stream_rational("resample_stream_rational_slots", x_new, kern, state, sd, consumed, orig, newf, width, hold, final,
                                     form)


def stream_samples(buf, fill, x_new, w, drop):
    """The sender's sample state in one launch (mvq_stream_samples_f32).  buf: contiguous fp32 [R, cap], the first ``fill`` samples
    of every row valid, updated in place; x_new [R, n].  With v = [buf[:, :fill] | x_new]: -> win[R, w] = v[:, :w], and
    buf[:, :fill + n - drop] = v[:, drop:].  w = 0 and drop = 0 is the pure append (an empty win comes back)."""
    x_new = _dev(x_new, "x_new")
    if not isinstance(buf, torch.Tensor) or buf.dim() != 2 or x_new.dim() != 2 or buf.dtype != torch.float32 or not buf.is_cuda \
            or not buf.is_contiguous() or buf.shape[0] != x_new.shape[0] or buf.device != x_new.device:
        raise MvqError("stream_samples: buf must be a contiguous fp32 HIP tensor [R, cap] with x_new's rows")
    R, cap = buf.shape
    n = x_new.shape[1]
    fill, w, drop = int(fill), int(w), int(drop)
    win = torch.empty(R, max(w, 0), device=buf.device, dtype=torch.float32)
    check(_lib.lib().mvq_stream_samples_f32(buf.data_ptr(), fill, x_new.data_ptr(), n, win.data_ptr(), w, drop, cap, R, _stream()),
          "mvq_stream_samples_f32")
    return win


def stream_samples_desc(sessions, w, cap, who="stream_samples_slots"):
    """Host only: the descriptor table of a group of pool sessions for mvq_stream_samples_slots_f32.  ``sessions``: host-integer
    tuples (slot, fill, n, drop); -> (rows [slot, fill, n, drop, x_off], x_total) with x_off the exclusive prefix sum of 2n, the
    packed layout of x_new.  Refuses every entry mvq_stream_samples_f32 would refuse for that ``w`` and ``cap`` (the slots are
    _slot_host's to check)."""
    rows, x_off = [], 0
    w, cap = int(w), int(cap)
    if w < 0 or not 0 <= cap <= 1 << 24:
        raise MvqError(f"{who}: w = {w}, cap = {cap}")
    for s in sessions:
        try:
            if isinstance(s, torch.Tensor) or len(s) != 4:
                raise TypeError
            slot, fill, n, drop = (operator.index(v) for v in s)
        except TypeError:
            raise MvqError(f"{who}: a session is four host integers (slot, fill, n, drop)") from None
        if fill < 0 or n < 0 or drop < 0 or n > 1 << 24:
            raise MvqError(f"{who}: slot {slot}: fill = {fill}, n = {n}, drop = {drop}")
        if fill > cap or fill + n - drop > cap:
            raise MvqError(f"{who}: slot {slot}: fill = {fill}, or the {fill + n - drop} samples to keep, exceed the capacity {cap}")
        if w > fill + n or drop > fill + n:
            raise MvqError(f"{who}: slot {slot}: w = {w} / drop = {drop} exceed fill + n = {fill} + {n}")
        rows.append([slot, fill, n, drop, x_off])
        x_off += 2 * n
    if x_off > 0x7FFFFFFF:
        raise MvqError(f"{who}: {x_off} new samples in one launch")
    return rows, x_off


def stream_samples_slots(buf, sessions, x_new, w, desc_dev=None):
    """stream_samples for a group of sessions of a sender pool, each with ITS fill, n and drop, in one launch
    (mvq_stream_samples_slots_f32).  buf: contiguous fp32 [S, 2, cap], slot s = the audio and the tactile row of one session,
    updated in place in the listed slots only.  ``sessions``: host-integer tuples (slot, fill, n, drop).  x_new: contiguous fp32,
    sum(2n) floats, per session its n new audio samples and then its n new tactile samples, in the order of ``sessions``.
    -> win[2, G, w]: the first w samples of [buf[slot, m, :fill] | new] of every session, audio rows then tactile rows (one w per
    launch; w = 0 with every drop 0 is the pure append).  ``desc_dev``: the int32 table [G, 5] of stream_samples_desc when the
    caller uploaded it already.  Everything is refused on the host, before anything is uploaded: a repeated or out-of-range slot,
    an entry stream_samples would refuse, an x_new of another size."""
    who = "stream_samples_slots"
    sessions = list(sessions) if not isinstance(sessions, torch.Tensor) else sessions
    pool_ok = isinstance(buf, torch.Tensor) and buf.dim() == 3 and buf.shape[1] == 2
    if not pool_ok:
        raise MvqError(f"{who}: buf must be a contiguous fp32 HIP tensor [slots, 2, cap]")
    rows, x_total = stream_samples_desc(sessions, w, buf.shape[2], who)
    _slot_host(who, [r[0] for r in rows], buf, 3)
    S, _, cap = buf.shape
    G, w = len(rows), int(w)
    if not isinstance(x_new, torch.Tensor) or x_new.dtype != torch.float32 or x_new.device != buf.device or not x_new.is_contiguous() \
            or x_new.numel() != x_total:
        raise MvqError(f"{who}: x_new must be a contiguous fp32 tensor of sum(2n) = {x_total} floats on {buf.device}")
    if desc_dev is None:
        desc_dev = torch.tensor(rows, dtype=torch.int32).reshape(G, 5).to(buf.device)
    elif not isinstance(desc_dev, torch.Tensor) or desc_dev.dtype != torch.int32 or desc_dev.device != buf.device \
            or tuple(desc_dev.shape) != (G, 5) or not desc_dev.is_contiguous():
        raise MvqError(f"{who}: desc_dev must be the contiguous int32 tensor [{G}, 5] of the table on {buf.device}")
    win = torch.empty(2, G, w, device=buf.device, dtype=torch.float32)
    check(_lib.lib().mvq_stream_samples_slots_f32(buf.data_ptr(), desc_dev.data_ptr(), G, S, x_new.data_ptr(), x_total, win.data_ptr(),
                                                  w, cap, _stream()), "mvq_stream_samples_slots_f32")
    return win


# ---------------------------------------------------------------------------------- backward (row f1)
def pack_conv1d_dgrad(w: torch.Tensor) -> torch.Tensor:
    """Conv1d weight w[Cout,Cin,ks] -> packed image of its input-gradient conv (flip + transpose)."""
    w = _dev(w, "w")
    cout, cin, ks = w.shape
    wp = torch.empty(_lib.lib().mvq_conv1d_dgrad_packed_floats(cin, cout, ks), device=w.device, dtype=torch.float32)
    check(_lib.lib().mvq_conv1d_pack_dgrad_f32(w.data_ptr(), wp.data_ptr(), cin, cout, ks, _stream()),
          "mvq_conv1d_pack_dgrad_f32")
    return wp


def pack_conv_transpose1d_dgrad(w: torch.Tensor) -> torch.Tensor:
    """ConvTranspose1d weight w[Cin,Cout,ks] -> packed image of its input-gradient (a strided conv)."""
    w = _dev(w, "w")
    cin, cout, ks = w.shape
    wp = torch.empty(_lib.lib().mvq_conv1d_dgrad_packed_floats(cin, cout, ks), device=w.device, dtype=torch.float32)
    check(_lib.lib().mvq_conv_transpose1d_pack_dgrad_f32(w.data_ptr(), wp.data_ptr(), cin, cout, ks, _stream()),
          "mvq_conv_transpose1d_pack_dgrad_f32")
    return wp


def conv1d_dgrad(gy, wp_dgrad, cin, tin, ks, stride=1, dil=1, pad=0, dsnake_src=None, dsnake_alpha=None, residual=None):
    """gx[B,cin,tin] = dgrad-conv(gy) * dsnake(dsnake_src) + residual; layer described by its FORWARD geometry."""
    gy = _dev(gy, "gy")
    B, cout, tout = gy.shape
    gx = torch.empty(B, cin, tin, device=gy.device, dtype=torch.float32)
    check(_lib.lib().mvq_conv1d_dgrad_f32(gy.data_ptr(), wp_dgrad.data_ptr(), _p(dsnake_src), _p(dsnake_alpha),
                                          _p(residual), gx.data_ptr(), B, cin, tin, cout, tout, ks, stride, dil, pad,
                                          _stream()), "mvq_conv1d_dgrad_f32")
    return gx


# ------------------------------------------------------- parameter gradients of the decoder's layers (fine-tuning T_DEC)
def _ws(nbytes, device):
    """Caller-provided workspace of a native call: fp32 storage of at least nbytes (None when the call needs none)."""
    return torch.empty((nbytes + 3) // 4, device=device, dtype=torch.float32) if nbytes else None


def conv1d_wgrad(gy, a, ks, stride=1, dil=1, pad=0, transposed=False, snake_alpha=None):
    """Gradient of a conv weight in the torch layout of weight_v, the layer described by its FORWARD geometry: gy[B,cout,tout]
    the gradient at its output, a[B,cin,tin] its input -> dW[cout,cin,ks] (Conv1d) or dW[cin,cout,ks] (ConvTranspose1d, ks ==
    2*stride).  snake_alpha[cin]: ``a`` is the saved input of the Snake in front of the layer; Snake is applied while staging."""
    gy = _dev(gy, "gy"); a = _dev(a, "a")
    if gy.dim() != 3 or a.dim() != 3 or gy.shape[0] != a.shape[0]:
        raise MvqError(f"conv1d_wgrad: gy {tuple(gy.shape)} and a {tuple(a.shape)} must be [B, C, T] with one batch")
    B, cout, tout = gy.shape
    _, cin, tin = a.shape
    ks, stride, dil, pad = int(ks), int(stride), int(dil), int(pad)
    if transposed:
        if ks != 2 * stride:
            raise MvqError(f"conv1d_wgrad: transposed kernel {ks} != 2*stride ({stride}) is outside the path")
        base = (tin - 1) * stride - 2 * pad + ks
        ok = base <= tout < base + stride if tin else tout == 0
    else:
        ok = stride == 1 and tout == tin + 2 * pad - dil * (ks - 1)
    if not ok:
        raise MvqError(f"conv1d_wgrad: tout {tout} does not match tin {tin}, ks {ks}, stride {stride}, dil {dil}, pad {pad}")
    if snake_alpha is not None:
        snake_alpha = _dev(snake_alpha, "snake_alpha")
        if snake_alpha.numel() != cin:
            raise MvqError(f"conv1d_wgrad: snake_alpha has {snake_alpha.numel()} entries, the layer {cin} input channels")
    geo = (B, cin, tin, cout, tout, ks, stride, dil, pad, int(bool(transposed)))
    dw = torch.empty((cin, cout, ks) if transposed else (cout, cin, ks), device=gy.device, dtype=torch.float32)
    nbytes = _lib.lib().mvq_conv1d_wgrad_workspace_bytes(*geo)
    ws = _ws(nbytes, gy.device)
    check(_lib.lib().mvq_conv1d_wgrad_f32(gy.data_ptr(), a.data_ptr(), _p(snake_alpha), dw.data_ptr(), _p(ws), nbytes, *geo, _stream()),
          "mvq_conv1d_wgrad_f32")
    return dw


def snake_bwd(gs, x, alpha, residual=None, need_dalpha=True):
    """Backward of Snake1d: gs the gradient at its output, x its saved input -> (gx, dalpha[C] or None).  gx = gs * dsnake(x)/dx +
    residual is bit for bit what conv1d_dgrad's fused epilogue gives."""
    gs = _dev(gs, "gs"); x = _dev(x, "x"); alpha = _dev(alpha, "alpha")
    if gs.dim() != 3 or gs.shape != x.shape or alpha.numel() != gs.shape[1]:
        raise MvqError(f"snake_bwd: gs {tuple(gs.shape)}, x {tuple(x.shape)}, alpha {tuple(alpha.shape)} do not match [B, C, T] / [C]")
    if residual is not None:
        residual = _dev(residual, "residual")
        if residual.shape != gs.shape:
            raise MvqError(f"snake_bwd: residual shape {tuple(residual.shape)} != {tuple(gs.shape)}")
    B, C, T = gs.shape
    gx = torch.empty_like(gs)
    dalpha = torch.empty(C, device=gs.device, dtype=torch.float32) if need_dalpha else None
    nbytes = _lib.lib().mvq_channel_reduce_workspace_bytes(B, C, T) if need_dalpha else 0
    ws = _ws(nbytes, gs.device)
    check(_lib.lib().mvq_snake_bwd_f32(gs.data_ptr(), x.data_ptr(), alpha.data_ptr(), _p(residual), gx.data_ptr(), _p(dalpha), _p(ws),
                                       nbytes, B, C, T, _stream()), "mvq_snake_bwd_f32")
    return gx, dalpha


def bias_grad(gy):
    """db[C] = sum over items and tokens of gy[B, C, T], in a fixed order."""
    gy = _dev(gy, "gy")
    if gy.dim() != 3:
        raise MvqError(f"bias_grad: gy {tuple(gy.shape)} must be [B, C, T]")
    B, C, T = gy.shape
    db = torch.empty(C, device=gy.device, dtype=torch.float32)
    nbytes = _lib.lib().mvq_channel_reduce_workspace_bytes(B, C, T)
    ws = _ws(nbytes, gy.device)
    check(_lib.lib().mvq_bias_grad_f32(gy.data_ptr(), db.data_ptr(), _p(ws), nbytes, B, C, T, _stream()), "mvq_bias_grad_f32")
    return db


def weight_norm_bwd(dw, v, g, need_dg=True, need_dv=True):
    """Backward of weight_norm(v, g) over dim-0 rows: dw the gradient of the folded weight -> (dg like g, dv like v)."""
    dw = _dev(dw, "dw"); v = _dev(v, "v"); g = _dev(g, "g")
    if dw.shape != v.shape or v.dim() < 2 or g.numel() != v.shape[0]:
        raise MvqError(f"weight_norm_bwd: dw {tuple(dw.shape)}, v {tuple(v.shape)}, g {tuple(g.shape)} do not match")
    if not (need_dg or need_dv):
        raise MvqError("weight_norm_bwd: nothing asked for")
    rows = v.shape[0]
    dg = torch.empty_like(g) if need_dg else None
    dv = torch.empty_like(v) if need_dv else None
    check(_lib.lib().mvq_weight_norm_bwd_f32(dw.data_ptr(), v.data_ptr(), g.data_ptr(), _p(dg), _p(dv), rows, v.numel() // max(rows, 1),
                                             _stream()), "mvq_weight_norm_bwd_f32")
    return dg, dv


def mul_dtanh(g, y):
    g = _dev(g, "g"); y = _dev(y, "y")
    out = torch.empty_like(g)
    check(_lib.lib().mvq_mul_dtanh_f32(g.data_ptr(), y.data_ptr(), out.data_ptr(), g.numel(), _stream()), "mvq_mul_dtanh_f32")
    return out


# ------------------------------------------------------- backward of the reference-owned trainable modules (row f1)
def _fold_dims(x, folded_batch):
    B, C, T = x.shape
    if folded_batch is None:
        return B, C, T, 0, 0
    if B != 1 or T % folded_batch:
        raise MvqError("folded tensor must be [1, C, B*T]")
    T //= folded_batch
    return folded_batch, C, T, T, folded_batch * T


def layernorm_c_bwd(x, gamma, g, pe=None, eps=1e-5, folded_batch=None, need_gx=True):
    """-> (gx or None, dgamma, dbeta) for y = LayerNorm_C(x + pe)."""
    x = _dev(x, "x"); g = _dev(g, "g")
    B, C, T, sb, sc = _fold_dims(x, folded_batch)
    gx = torch.empty_like(x) if need_gx else None
    dgamma = torch.zeros(C, device=x.device, dtype=torch.float32)
    dbeta = torch.zeros(C, device=x.device, dtype=torch.float32)
    stats = torch.empty(2 * max(B * T, 1), device=x.device, dtype=torch.float32)
    check(_lib.lib().mvq_layernorm_c_bwd_f32(x.data_ptr(), _p(pe), gamma.data_ptr(), g.data_ptr(), _p(gx),
                                             dgamma.data_ptr(), dbeta.data_ptr(), stats.data_ptr(), B, C, T, sb, sc,
                                             float(eps), _stream()), "mvq_layernorm_c_bwd_f32")
    return gx, dgamma, dbeta


def gelu_bwd(x, g):
    x = _dev(x, "x"); g = _dev(g, "g")
    gx = torch.empty_like(x)
    check(_lib.lib().mvq_gelu_bwd_f32(x.data_ptr(), g.data_ptr(), gx.data_ptr(), x.numel(), _stream()), "mvq_gelu_bwd_f32")
    return gx


def scale_tanh(u, scale: float):
    u = _dev(u, "u")
    y = torch.empty_like(u)
    check(_lib.lib().mvq_scale_tanh_f32(u.data_ptr(), float(scale), y.data_ptr(), u.numel(), _stream()), "mvq_scale_tanh_f32")
    return y


def scale_tanh_bwd(u, g, scale: float):
    """-> (gu, d/dscale as a 0-d device tensor)."""
    u = _dev(u, "u"); g = _dev(g, "g")
    gu = torch.empty_like(u)
    nblk = max(1, min(1024, (u.numel() + 255) // 256))
    partial = torch.zeros(nblk, device=u.device, dtype=torch.float32)
    check(_lib.lib().mvq_scale_tanh_bwd_f32(u.data_ptr(), g.data_ptr(), float(scale), gu.data_ptr(), partial.data_ptr(),
                                            nblk, u.numel(), _stream()), "mvq_scale_tanh_bwd_f32")
    dscale = torch.empty(1, device=u.device, dtype=torch.float32)
    check(_lib.lib().mvq_rowsum_f32(partial.data_ptr(), dscale.data_ptr(), 1, nblk, 0, _stream()), "mvq_rowsum_f32")
    return gu, dscale.reshape(())


def attention_bwd(q, k, v, g, heads, folded_batch=None, kmask=None, m_stride=None):
    """-> (gq, gk, gv) of ``attention``.  ``kmask`` / ``m_stride`` as there: mvq_attention_masked_bwd_f32 -- gq, and gk / gv at
    the present columns, are this call's on the compacted K / V bit for bit; gk / gv at an absent column are +0."""
    q = _dev(q, "q"); k = _dev(k, "k"); v = _dev(v, "v"); g = _dev(g, "g")
    B, C, Tq = q.shape
    Tk = k.shape[2]
    strides = (0, 0, 0, 0)
    if folded_batch is not None:
        B = folded_batch
        Tq, Tk = Tq // B, Tk // B
        strides = (Tq, B * Tq, Tk, B * Tk)
    gq, gk, gv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    if kmask is not None:
        kmask, ms = _chunk_key_mask("attention_bwd", kmask, m_stride, B, Tk, q.device)
        check(_lib.lib().mvq_attention_masked_bwd_f32(q.data_ptr(), k.data_ptr(), v.data_ptr(), kmask.data_ptr(), g.data_ptr(),
                                                      gq.data_ptr(), gk.data_ptr(), gv.data_ptr(), B, heads, C // heads, Tq, Tk,
                                                      *strides, ms, _stream()), "mvq_attention_masked_bwd_f32")
        return gq, gk, gv
    check(_lib.lib().mvq_attention_bwd_f32(q.data_ptr(), k.data_ptr(), v.data_ptr(), g.data_ptr(), gq.data_ptr(),
                                           gk.data_ptr(), gv.data_ptr(), B, heads, C // heads, Tq, Tk, *strides,
                                           _stream()), "mvq_attention_bwd_f32")
    return gq, gk, gv


def mul_scaled(a, b, scale=1.0):
    a = _dev(a, "a"); b = _dev(b, "b")
    out = torch.empty_like(a)
    check(_lib.lib().mvq_mul_scaled_f32(a.data_ptr(), b.data_ptr(), float(scale), out.data_ptr(), a.numel(), _stream()),
          "mvq_mul_scaled_f32")
    return out


def transpose2d(x):
    x = _dev(x, "x")
    r, c = x.shape
    out = torch.empty(c, r, device=x.device, dtype=torch.float32)
    check(_lib.lib().mvq_transpose2d_f32(x.data_ptr(), out.data_ptr(), r, c, _stream()), "mvq_transpose2d_f32")
    return out


def rowsum(x):
    x = _dev(x, "x")
    r, c = x.shape
    out = torch.empty(r, device=x.device, dtype=torch.float32)
    check(_lib.lib().mvq_rowsum_f32(x.data_ptr(), out.data_ptr(), r, c, 0, _stream()), "mvq_rowsum_f32")
    return out


def linear_wgrad(g, x):
    """dW[O,I] = g[O,N] x[I,N]^T over the token axis N, as a k=1 conv on the MFMA kernel with K = tokens:
    packed 'weights' = g^T (K-major), input = x^T [N, I].  N is padded with zero tokens to a multiple of 32."""
    g = _dev(g, "g"); x = _dev(x, "x")
    O, N = g.shape
    I, N2 = x.shape
    if N != N2:
        raise MvqError("linear_wgrad: token counts differ")
    if N % 32:
        padn = 32 - N % 32
        g = torch.nn.functional.pad(g, (0, padn)); x = torch.nn.functional.pad(x, (0, padn)); N += padn
    wp = pack_conv1d(g.reshape(O, N, 1))
    xt = transpose2d(x).reshape(1, N, I)
    return conv1d(xt, wp, O, 1).reshape(O, I)


# ---------------------------------------------------------------------------------------- training losses (row f2)
def stft_frames(x, window, out, col0, n_fft, hop):
    """x[B,T] -> out[n_fft, ncols][:, col0 : col0 + B*nframes] (windowed, reflect-padded, center=True)."""
    B, T = x.shape
    nfr = 1 + T // hop
    check(_lib.lib().mvq_stft_frames_f32(x.data_ptr(), window.data_ptr(), out.data_ptr(), B, T, n_fft, hop, nfr,
                                         out.shape[1], col0, _stream()), "mvq_stft_frames_f32")


def spec_mag(S, F, Fp, eps):
    ncols = S.shape[-1]
    mag = torch.empty(Fp, ncols, device=S.device, dtype=torch.float32)
    check(_lib.lib().mvq_spec_mag_f32(S.data_ptr(), mag.data_ptr(), F, Fp, ncols, float(eps), _stream()), "mvq_spec_mag_f32")
    return mag


def spec_loss_sums(mag, F, B, nfr):
    """-> [3, B]: per item sums of (X-Y)^2, Y^2, |X-Y|."""
    P = 16
    partial = torch.empty(3 * B, P, device=mag.device, dtype=torch.float32)
    check(_lib.lib().mvq_spec_loss_partial_f32(mag.data_ptr(), partial.data_ptr(), P, F, B, nfr, mag.shape[1], _stream()),
          "mvq_spec_loss_partial_f32")
    return rowsum(partial).reshape(3, B)


def spec_grad(S, mag, coef_a, coef_b, extra, F, Fp, B, nfr, eps):
    G = torch.empty(2 * Fp, B * nfr, device=S.device, dtype=torch.float32)
    check(_lib.lib().mvq_spec_grad_f32(S.data_ptr(), mag.data_ptr(), _p(coef_a), float(coef_b), _p(extra), G.data_ptr(),
                                       F, Fp, B, nfr, mag.shape[1], float(eps), _stream()), "mvq_spec_grad_f32")
    return G


def overlap_add_(dy, dframes, window, n_fft, hop):
    B, T = dy.shape
    check(_lib.lib().mvq_overlap_add_f32(dframes.data_ptr(), window.data_ptr(), dy.data_ptr(), B, T, n_fft, hop,
                                         1 + T // hop, _stream()), "mvq_overlap_add_f32")
    return dy


def l1_loss_sum(y, tgt, dy=None, coef=0.0):
    """sum |finite_or_zero(y) - finite_or_zero(tgt)| (0-d device tensor); dy += coef*sign(...) when dy is given."""
    n = y.numel()
    P = max(1, min(1024, (n + 255) // 256))
    partial = torch.empty(1, P, device=y.device, dtype=torch.float32)
    check(_lib.lib().mvq_l1_loss_f32(y.data_ptr(), tgt.data_ptr(), partial.data_ptr(), P, _p(dy), float(coef), n, _stream()),
          "mvq_l1_loss_f32")
    return rowsum(partial).reshape(())


def mel_max(M, n_mels, B, nfr):
    maxv = torch.empty(2 * B, device=M.device, dtype=torch.float32)
    argm = torch.empty(2 * B, device=M.device, dtype=torch.int32)
    check(_lib.lib().mvq_mel_max_f32(M.data_ptr(), maxv.data_ptr(), argm.data_ptr(), n_mels, B, nfr, M.shape[-1], _stream()),
          "mvq_mel_max_f32")
    return maxv, argm


def mel_cos(M, maxv, n_mels, B, nfr, eps, coef=None, use_log=True):
    """-> cos[B*nfr] (, dM[n_mels, B*nfr], dden[B*nfr] when coef = dL/dcos is given)."""
    cosv = torch.empty(B * nfr, device=M.device, dtype=torch.float32)
    dM = torch.empty(n_mels, B * nfr, device=M.device, dtype=torch.float32) if coef is not None else None
    dden = torch.empty(B * nfr, device=M.device, dtype=torch.float32) if coef is not None else None
    check(_lib.lib().mvq_mel_cos_f32(M.data_ptr(), maxv.data_ptr(), cosv.data_ptr(), _p(dM), _p(dden),
                                     float(coef or 0.0), n_mels, B, nfr, M.shape[-1], float(eps), int(use_log), _stream()),
          "mvq_mel_cos_f32")
    return cosv, dM, dden


def mel_max_grad_(dM, dden, maxv, argm, B, nfr, eps):
    check(_lib.lib().mvq_mel_max_grad_f32(dden.data_ptr(), maxv.data_ptr(), argm.data_ptr(), dM.data_ptr(), B, nfr, float(eps),
                                          _stream()), "mvq_mel_max_grad_f32")
    return dM


# ---------------------------------------------------------------------------------------- whole stacks (include/mvq.h, ABI 3)
class Stack:
    """mvq_stack handle of one dac Encoder / Decoder: launch plan + folded / packed weights in one device blob.

    ``Stack.encoder(d_model, strides, d_latent)`` / ``Stack.decoder(input_channel, channels, rates, d_out, output_padding)`` make a
    description-only handle (``param_names()`` lists the upstream state-dict keys it expects, in order); ``bind(tensors)`` makes
    the working handle from the parameter tensors in that order.  ``encoder_fwd`` / ``decoder_fwd`` / ``decoder_fwd_saving`` /
    ``decoder_bwd_input`` are ONE C call each (mvq_encoder_fwd_f32, ...): the per-layer plan lives in the library."""

    _BY_ID = {}                      # torch.ops.mi355x_vqvae.encoder_fwd / decoder_fwd / decoder_bwd_input name a stack by this id

    def __init__(self, kind, desc, handle, blob=None):
        import weakref
        self.kind, self.desc, self.handle, self.blob = kind, desc, handle, blob
        self._ws_bytes = {}          # (batch, t) -> mvq_*_workspace_bytes: the query walks the plan, so it runs once per shape
        self.id = id(self)
        Stack._BY_ID[self.id] = weakref.ref(self)

    def __deepcopy__(self, memo):            # a handle is not copied with its module: the copy rebuilds its own on first use
        return None

    def __reduce__(self):                    # ... nor pickled (torch.save(module)): it pickles as None
        return (type(None), ())

    @classmethod
    def by_id(cls, i):
        ref = cls._BY_ID.get(int(i))
        st = ref() if ref else None
        if st is None:
            raise MvqError(f"no live Stack with id {i}")
        return st

    @classmethod
    def _make(cls, kind, desc, params=None):
        import ctypes
        L = _lib.lib()
        create = L.mvq_encoder_create if kind == "encoder" else L.mvq_decoder_create
        h = ctypes.c_void_p()
        if params is None:
            check(create(ctypes.byref(h), ctypes.byref(desc), None, None, 0, None), f"mvq_{kind}_create")
            return cls(kind, desc, h)
        probe = cls._make(kind, desc)
        names = probe.param_names()
        if len(params) != len(names):
            raise MvqError(f"Stack.bind: {len(params)} tensors for {len(names)} parameters")
        ts = [_dev(p.detach(), n) for p, n in zip(params, names)]
        for t, (n, shp) in zip(ts, probe.param_info()):
            if t.numel() != shp[0] * shp[1] * shp[2]:
                raise MvqError(f"Stack.bind: {n} has {t.numel()} elements, expected shape {shp}")
        blob = torch.empty(int(L.mvq_stack_weights_bytes(probe.handle)), device=ts[0].device, dtype=torch.uint8)
        arr = (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
        check(create(ctypes.byref(h), ctypes.byref(desc), arr, blob.data_ptr(), blob.numel(), _stream()), f"mvq_{kind}_create")
        return cls(kind, desc, h, blob)

    @classmethod
    def encoder(cls, d_model, strides, d_latent, params=None):
        d = _lib.EncoderDesc()
        d.d_model, d.n_strides, d.d_latent = int(d_model), len(strides), int(d_latent)
        for i, s in enumerate(strides):
            d.strides[i] = int(s)
        return cls._make("encoder", d, params)

    @classmethod
    def decoder(cls, input_channel, channels, rates, d_out=1, output_padding=False, params=None):
        d = _lib.DecoderDesc()
        d.input_channel, d.channels, d.n_rates, d.d_out, d.output_padding = int(input_channel), int(channels), len(rates), int(d_out), int(bool(output_padding))
        for i, s in enumerate(rates):
            d.rates[i] = int(s)
        return cls._make("decoder", d, params)

    def bind(self, params):
        return Stack._make(self.kind, self.desc, list(params))

    def __del__(self):
        try:
            Stack._BY_ID.pop(getattr(self, "id", None), None)
            if self.handle:
                _lib.lib().mvq_stack_destroy(self.handle)
                self.handle = None
        except Exception:
            pass

    def param_info(self):
        import ctypes
        L = _lib.lib()
        out = []
        for i in range(L.mvq_stack_param_count(self.handle)):
            buf = ctypes.create_string_buffer(128)
            dims = (ctypes.c_int * 3)()
            check(L.mvq_stack_param_info(self.handle, i, buf, 128, dims), "mvq_stack_param_info")
            out.append((buf.value.decode(), tuple(dims)))
        return out

    def param_names(self):
        return [n for n, _ in self.param_info()]

    def set_plan(self, vpack_min_batch=0, pack_min_batch=0):
        check(_lib.lib().mvq_stack_set_plan(self.handle, int(vpack_min_batch), int(pack_min_batch)), "mvq_stack_set_plan")
        self._ws_bytes.clear()                                   # the thresholds change the plans, hence their workspace

    def out_len(self, t):
        L = _lib.lib()
        return int(L.mvq_encoder_out_len(self.handle, int(t)) if self.kind == "encoder" else L.mvq_decoder_out_len(self.handle, int(t)))

    def _ws(self, x, B, t):
        n = self._ws_bytes.get((B, t))
        if n is None:
            L = _lib.lib()
            query = L.mvq_encoder_workspace_bytes if self.kind == "encoder" else L.mvq_decoder_workspace_bytes
            n = self._ws_bytes[(B, t)] = max(int(query(self.handle, B, t)), 256)
        return torch.empty(n, device=x.device, dtype=torch.uint8)

    def encoder_fwd(self, x):
        """x[B, 1, T] -> z[B, d_latent, Tl]: mvq_encoder_fwd_f32."""
        x = _dev(x, "x")
        B, _, T = x.shape
        z = torch.empty(B, self.desc.d_latent, max(self.out_len(T), 0), device=x.device, dtype=torch.float32)
        if z.numel():
            ws = self._ws(x, B, T)
            check(_lib.lib().mvq_encoder_fwd_f32(self.handle, x.data_ptr(), z.data_ptr(), ws.data_ptr(), ws.numel(), B, T, _stream()), "mvq_encoder_fwd_f32")
        return z

    def decoder_fwd(self, z):
        """z[B, C, t] -> y[B, d_out, Tout] (tanh applied): mvq_decoder_fwd_f32."""
        z = _dev(z, "z")
        B, _, t = z.shape
        y = torch.empty(B, self.desc.d_out, max(self.out_len(t), 0), device=z.device, dtype=torch.float32)
        if y.numel():
            ws = self._ws(z, B, t)
            check(_lib.lib().mvq_decoder_fwd_f32(self.handle, z.data_ptr(), y.data_ptr(), ws.data_ptr(), ws.numel(), B, t, _stream()), "mvq_decoder_fwd_f32")
        return y

    # ---- stateful streaming decode (include/mvq.h)
    def decoder_stream_state_floats(self):
        return int(_lib.lib().mvq_decoder_stream_state_floats(self.handle))

    def decoder_stream_state(self, rows, device=None):
        """The state of ``rows`` streaming sessions: fp32 [rows, S], every stage's tail at a fixed offset of a row.  Not cleared: a new
        session reads none of it."""
        S = self.decoder_stream_state_floats()
        if self.kind != "decoder" or S == 0:
            raise MvqError("Stack.decoder_stream_state: not a decoder stack the stage plan covers")
        if int(rows) < 1:
            raise MvqError("Stack.decoder_stream_state: rows must be at least 1")
        return torch.empty(int(rows), S, device=self.blob.device if device is None else device, dtype=torch.float32)

    def decoder_stream_plan(self, tokens_before, n, last=False):
        """-> (stages, (e0, e1)): per stage (h_in, src_off, n_new, h_out, cap) of the step (mvq_decoder_stream_plan, host only)."""
        import ctypes
        L = _lib.lib()
        ns = int(L.mvq_decoder_stream_plan(self.handle, 0, 0, 0, None, 0, None))
        if ns <= 0:
            check(ns or -2, "mvq_decoder_stream_plan")
        buf, emit = (ctypes.c_int32 * (5 * ns))(), (ctypes.c_int32 * 2)()
        rc = int(L.mvq_decoder_stream_plan(self.handle, int(tokens_before), int(n), int(bool(last)), buf, ns, emit))
        if rc < 0:
            check(rc, "mvq_decoder_stream_plan")
        return tuple(tuple(buf[5 * k:5 * k + 5]) for k in range(ns)), (int(emit[0]), int(emit[1]))

    def decoder_stream_fwd(self, state, z_new, tokens_before, last=False, slots=None, slots_dev=None):
        """One step of the stateful decoder: z_new[G, C, n] after ``tokens_before`` tokens -> y[G, d_out, n_emit] (mvq_decoder_stream_fwd_f32);
        ``state`` (decoder_stream_state) moves on in place.  ``slots`` None: session g is state row g; else host integers, session
        g on state[slots[g]] (``slots_dev``: their int32 device copy when the caller uploaded it already).  Only arithmetic mode
        "f32" (the opt-in modes scale per item)."""
        if get_arith() != "f32":
            raise ValueError(f"Stack.decoder_stream_fwd: arithmetic mode {get_arith()!r} scales per item; only 'f32' is equal piece by piece")
        S = self.decoder_stream_state_floats()
        if not isinstance(state, torch.Tensor) or state.dim() != 2 or state.shape[1] != S or state.dtype != torch.float32:
            raise ValueError(f"Stack.decoder_stream_fwd: the state must be an fp32 tensor [sessions, {S}] (decoder_stream_state), got "
                             f"{tuple(state.shape) if isinstance(state, torch.Tensor) else type(state).__name__}")
        z_new = _dev(z_new, "z_new")
        if not state.is_cuda or not state.is_contiguous() or state.device != z_new.device:
            raise ValueError("Stack.decoder_stream_fwd: the state must be contiguous and on z_new's device")
        if z_new.dim() != 3 or z_new.shape[1] != self.desc.input_channel:
            raise ValueError(f"Stack.decoder_stream_fwd: z_new must be [G, {self.desc.input_channel}, n], got {tuple(z_new.shape)}")
        G, _, n = z_new.shape
        sd = None
        if slots is not None:
            g, sd = _slot_list("Stack.decoder_stream_fwd", slots, state, 2, slots_dev)
            if g != G:
                raise ValueError(f"Stack.decoder_stream_fwd: {g} slots for {G} sessions")
        elif G > state.shape[0]:
            raise ValueError(f"Stack.decoder_stream_fwd: {G} sessions, the state has {state.shape[0]} rows")
        before, last = int(tokens_before), bool(last)
        _, (e0, e1) = self.decoder_stream_plan(before, n, last)
        y = torch.empty(G, self.desc.d_out, e1 - e0, device=z_new.device, dtype=torch.float32)
        if G == 0:
            return y
        key = ("stream", G, min(before, 16), n, last)
        nb = self._ws_bytes.get(key)
        if nb is None:
            nb = self._ws_bytes[key] = max(int(_lib.lib().mvq_decoder_stream_workspace_bytes(self.handle, G, before, n, int(last))), 256)
        ws = torch.empty(nb, device=z_new.device, dtype=torch.uint8)
        check(_lib.lib().mvq_decoder_stream_fwd_f32(self.handle, state.data_ptr(), None if sd is None else sd.data_ptr(), G, state.shape[0],
                                                    z_new.data_ptr(), n, before, int(last), y.data_ptr(), e1 - e0, ws.data_ptr(), ws.numel(),
                                                    _stream()), "mvq_decoder_stream_fwd_f32")
        return y

    # ---- stateful streaming encode (include/mvq.h)
    def encoder_stream_state_floats(self):
        return int(_lib.lib().mvq_encoder_stream_state_floats(self.handle))

    def encoder_stream_state(self, rows, device=None):
        """The state of ``rows`` streaming sender sessions: fp32 [rows, S], every stage's raw tail at a fixed offset of a row.  Not
        cleared: a new session reads none of it."""
        S = self.encoder_stream_state_floats()
        if self.kind != "encoder" or S == 0:
            raise MvqError("Stack.encoder_stream_state: not an encoder stack the stage plan covers")
        if int(rows) < 1:
            raise MvqError("Stack.encoder_stream_state: rows must be at least 1")
        return torch.empty(int(rows), S, device=self.blob.device if device is None else device, dtype=torch.float32)

    def encoder_stream_plan(self, samples_before, n, last=False):
        """-> (stages, (t0, t1)): per stage (h_in, src_off, n_new, h_out, cap) of the step and the global latent columns it emits
        (mvq_encoder_stream_plan, host only)."""
        import ctypes
        L = _lib.lib()
        ns = int(L.mvq_encoder_stream_plan(self.handle, 0, 0, 0, None, 0, None))
        if ns <= 0:
            check(ns or -2, "mvq_encoder_stream_plan")
        buf, emit = (ctypes.c_int32 * (5 * ns))(), (ctypes.c_longlong * 2)()
        rc = int(L.mvq_encoder_stream_plan(self.handle, int(samples_before), int(n), int(bool(last)), buf, ns, emit))
        if rc < 0:
            check(rc, "mvq_encoder_stream_plan")
        return tuple(tuple(buf[5 * k:5 * k + 5]) for k in range(ns)), (int(emit[0]), int(emit[1]))

    def encoder_stream_fwd(self, state, x_new, samples_before, last=False, slots=None, slots_dev=None):
        """One step of the stateful encoder: x_new[G, 1, n] after ``samples_before`` samples -> z[G, d_latent, n_emit]
        (mvq_encoder_stream_fwd_f32); ``state`` (encoder_stream_state) moves on in place.  ``slots`` None: session g is state row g;
        else host integers, session g on state[slots[g]] (``slots_dev``: their int32 device copy when the caller uploaded it
        already).  Only arithmetic mode "f32" (the opt-in modes scale per item)."""
        if get_arith() != "f32":
            raise ValueError(f"Stack.encoder_stream_fwd: arithmetic mode {get_arith()!r} scales per item; only 'f32' is equal piece by piece")
        S = self.encoder_stream_state_floats()
        if not isinstance(state, torch.Tensor) or state.dim() != 2 or state.shape[1] != S or state.dtype != torch.float32:
            raise ValueError(f"Stack.encoder_stream_fwd: the state must be an fp32 tensor [sessions, {S}] (encoder_stream_state), got "
                             f"{tuple(state.shape) if isinstance(state, torch.Tensor) else type(state).__name__}")
        x_new = _dev(x_new, "x_new")
        if not state.is_cuda or not state.is_contiguous() or state.device != x_new.device:
            raise ValueError("Stack.encoder_stream_fwd: the state must be contiguous and on x_new's device")
        if x_new.dim() != 3 or x_new.shape[1] != 1:
            raise ValueError(f"Stack.encoder_stream_fwd: x_new must be [G, 1, n], got {tuple(x_new.shape)}")
        G, _, n = x_new.shape
        sd = None
        if slots is not None:
            g, sd = _slot_list("Stack.encoder_stream_fwd", slots, state, 2, slots_dev)
            if g != G:
                raise ValueError(f"Stack.encoder_stream_fwd: {g} slots for {G} sessions")
        elif G > state.shape[0]:
            raise ValueError(f"Stack.encoder_stream_fwd: {G} sessions, the state has {state.shape[0]} rows")
        before, last = int(samples_before), bool(last)
        stages, (t0, t1) = self.encoder_stream_plan(before, n, last)
        z = torch.empty(G, self.desc.d_latent, t1 - t0, device=x_new.device, dtype=torch.float32)
        if G == 0:
            return z
        key = ("enc_stream", G, stages, last)                     # the launches are a function of the plan alone
        nb = self._ws_bytes.get(key)
        if nb is None:
            nb = self._ws_bytes[key] = max(int(_lib.lib().mvq_encoder_stream_workspace_bytes(self.handle, G, before, n, int(last))), 256)
        ws = torch.empty(nb, device=x_new.device, dtype=torch.uint8)
        check(_lib.lib().mvq_encoder_stream_fwd_f32(self.handle, state.data_ptr(), None if sd is None else sd.data_ptr(), G, state.shape[0],
                                                    x_new.data_ptr(), n, before, int(last), z.data_ptr(), t1 - t0, ws.data_ptr(), ws.numel(),
                                                    _stream()), "mvq_encoder_stream_fwd_f32")
        return z

    def decoder_fwd_saving(self, z):
        """-> (y, saved): the training forward; `saved` (one uint8 tensor) goes to decoder_bwd_input."""
        z = _dev(z, "z")
        B, _, t = z.shape
        L = _lib.lib()
        y = torch.empty(B, self.desc.d_out, self.out_len(t), device=z.device, dtype=torch.float32)
        saved = torch.empty(int(L.mvq_decoder_saved_bytes(self.handle, B, t)), device=z.device, dtype=torch.uint8)
        ws = self._ws(z, B, t)
        check(L.mvq_decoder_fwd_saving_f32(self.handle, z.data_ptr(), y.data_ptr(), saved.data_ptr(), saved.numel(), ws.data_ptr(), ws.numel(), B, t,
                                           _stream()), "mvq_decoder_fwd_saving_f32")
        return y, saved

    def decoder_bwd_input(self, saved, gy, batch, t):
        """dL/dz [batch, C, t] from dL/dy and the saved forward: mvq_decoder_bwd_input_f32."""
        gy = _dev(gy, "gy")
        gz = torch.empty(batch, self.desc.input_channel, t, device=gy.device, dtype=torch.float32)
        ws = self._ws(gy, batch, t)
        check(_lib.lib().mvq_decoder_bwd_input_f32(self.handle, saved.data_ptr(), saved.numel(), gy.data_ptr(), gz.data_ptr(), ws.data_ptr(), ws.numel(),
                                                   batch, t, _stream()), "mvq_decoder_bwd_input_f32")
        return gz
