"""Autograd for the reference's trainable head: torch.autograd.Function wrappers whose
forward AND backward run on libmvq_hip.so, so that the reference's own training step

    out = net.forward_step(a, tc); total = ...losses(out["y_hat"], out["tgt"]); total.backward(); opt.step()

(Training/compare_dacvsproposal_5.py:379-396) works unchanged on the drop-in modules: the trainable parameters are
exactly the reference's (CrossPredictor, TokenNorm, scale, proj_down, proj_up; vq.books are EMA-updated, never by
gradient, ...:367), the frozen DAC decoder passes the gradient through (dac.Decoder.backward_input), and the encoders
and audio quantiser run without a graph, as in the reference where their outputs carry no gradient path to a
trainable tensor.

All tensors here are in the token-folded layout [1, C, B*n] of proposed._ar_latents.  Parity bar: gradients equal
torch autograd on the torch restatement within fp32 tolerance (tests/test_gpu_train.py); the forward values are the
bit-exact inference kernels.
"""
from __future__ import annotations

import torch

from . import ops

Function = torch.autograd.Function


def _c(g):
    return g.contiguous() if g is not None else None


class Linear(Function):
    """y = W x + b (+ residual) over folded tokens.  W is [O, I] or [O, I, 1]."""

    @staticmethod
    def forward(ctx, x, w, b, residual, packed):
        y = packed(x.detach(), residual=residual.detach() if residual is not None else None)
        ctx.save_for_backward(x, w)
        ctx.has_b, ctx.has_res = b is not None, residual is not None
        ctx.packed = packed if (hasattr(packed, "wp_dgrad") and getattr(getattr(packed, "mod", None), "weight", None) is w) else None
        return y

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        g = _c(g)
        O, I = w.shape[0], w.shape[1]
        N = g.shape[-1]
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            wp = ctx.packed.wp_dgrad() if ctx.packed is not None else ops.pack_conv1d_dgrad(w.detach().reshape(O, I, 1))
            gx = ops.conv1d_dgrad(g, wp, I, N, 1)
        if ctx.needs_input_grad[1]:
            gw = ops.linear_wgrad(g.reshape(O, N), x.detach().reshape(I, N)).reshape(w.shape)
        if ctx.has_b and ctx.needs_input_grad[2]:
            gb = ops.rowsum(g.reshape(O, N))
        gres = g if (ctx.has_res and ctx.needs_input_grad[3]) else None
        return gx, gw, gb, gres, None


class LayerNormC(Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, pe, eps, fb):
        y = ops.layernorm_c(x.detach(), gamma.detach(), beta.detach(), pe=pe, eps=eps, folded_batch=fb)
        ctx.save_for_backward(x, gamma)
        ctx.pe, ctx.eps, ctx.fb = pe, eps, fb
        return y

    @staticmethod
    def backward(ctx, g):
        x, gamma = ctx.saved_tensors
        gx, dg, db = ops.layernorm_c_bwd(x.detach(), gamma.detach(), _c(g), pe=ctx.pe, eps=ctx.eps, folded_batch=ctx.fb,
                                         need_gx=ctx.needs_input_grad[0])
        return gx, dg, db, None, None, None


class Gelu(Function):
    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return ops.gelu(x.detach())

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return ops.gelu_bwd(x.detach(), _c(g))


class Attention(Function):
    """``kmask`` (optional, uint8 [B, Tk], nonzero = key present) is not differentiated."""

    @staticmethod
    def forward(ctx, q, k, v, heads, fb, kmask=None):
        ctx.save_for_backward(q, k, v)
        ctx.heads, ctx.fb, ctx.kmask = heads, fb, kmask
        if kmask is None:
            return ops.attention(q.detach(), k.detach(), v.detach(), heads, folded_batch=fb)
        return ops.attention(q.detach(), k.detach(), v.detach(), heads, folded_batch=fb, kmask=kmask)

    @staticmethod
    def backward(ctx, g):
        q, k, v = ctx.saved_tensors
        if ctx.kmask is None:
            gq, gk, gv = ops.attention_bwd(q.detach(), k.detach(), v.detach(), _c(g), ctx.heads, folded_batch=ctx.fb)
        else:
            gq, gk, gv = ops.attention_bwd(q.detach(), k.detach(), v.detach(), _c(g), ctx.heads, folded_batch=ctx.fb, kmask=ctx.kmask)
        return gq, gk, gv, None, None, None


class AttentionSeq(Function):
    """Full-sequence attention (ops.attention_seq / attention_seq_bwd): the PLC predictor's call over all T_lat tokens."""

    @staticmethod
    def forward(ctx, q, k, v, heads, fb, kmask=None):
        ctx.save_for_backward(q, k, v)
        ctx.heads, ctx.fb, ctx.kmask = heads, fb, kmask
        return ops.attention_seq(q.detach(), k.detach(), v.detach(), heads, folded_batch=fb, kmask=kmask)

    @staticmethod
    def backward(ctx, g):
        q, k, v = ctx.saved_tensors
        gq, gk, gv = ops.attention_seq_bwd(q.detach(), k.detach(), v.detach(), _c(g), ctx.heads, folded_batch=ctx.fb, kmask=ctx.kmask)
        return gq, gk, gv, None, None, None


class PlcFill(Function):
    """z_filled = where(mask, z_pred, zt * ~mask) (PLC/PLC1.py:401-410); the gradient reaches z_pred only (zt comes from
    the frozen encoder)."""

    @staticmethod
    def forward(ctx, zt, z_pred, mask, fb):
        ctx.mask, ctx.fb = mask, fb
        return ops.plc_mask_fill(zt.detach(), z_pred.detach(), mask, folded_batch=fb, want_zt_in=False)[1]

    @staticmethod
    def backward(ctx, g):
        gz = ops.plc_mask_fill_bwd(_c(g), ctx.mask, folded_batch=ctx.fb) if ctx.needs_input_grad[1] else None
        return None, gz, None, None


class Dropout(Function):
    """x * mask / (1-p); the keep-mask comes from torch's generator (as nn.Dropout's does), the multiply is ours."""

    @staticmethod
    def forward(ctx, x, p):
        mask = torch.empty_like(x).bernoulli_(1.0 - p)
        ctx.mask, ctx.k = mask, 1.0 / (1.0 - p)
        return ops.mul_scaled(x.detach(), mask, ctx.k)

    @staticmethod
    def backward(ctx, g):
        return ops.mul_scaled(_c(g), ctx.mask, ctx.k), None


class ScaleTanh(Function):
    """y = clamp(scale, 5e-3, 0.5) * tanh(u)   (Training/...5.py:313-315)."""

    LO, HI = 5e-3, 0.5

    @staticmethod
    def forward(ctx, u, scale, raw=None):
        if raw is None:                                   # one device read; callers in a loop pass the cached host value
            raw = float(scale.detach().float().item())
        s = min(max(raw, ScaleTanh.LO), ScaleTanh.HI)
        ctx.save_for_backward(u)
        ctx.s, ctx.inside = s, (ScaleTanh.LO <= raw <= ScaleTanh.HI)
        return ops.scale_tanh(u.detach(), s)

    @staticmethod
    def backward(ctx, g):
        (u,) = ctx.saved_tensors
        gu, ds = ops.scale_tanh_bwd(u.detach(), _c(g), ctx.s)
        if not ctx.inside:
            ds = torch.zeros_like(ds)
        return gu, ds, None


class RvqSte(Function):
    """ResidualVQEMA.forward with its straight-through estimator: every stage adds `residual` back with gradient 1 and
    every stage's residual is the input minus detached codes, so d out / d z = (number of books used) * I
    (Training/...5.py:262-265)."""

    @staticmethod
    def forward(ctx, z, books, n_use):
        nb = books.shape[0] if n_use is None else max(0, min(int(n_use), books.shape[0]))
        ctx.nb = nb
        return ops.rvq_ema_forward(z.detach(), books, n_use)

    @staticmethod
    def backward(ctx, g):
        return g * float(ctx.nb), None, None


class RvqSteLayers(Function):
    """The layered straight-through quantiser of the training step under a lossy link: the full greedy search (whose first m
    indices do not depend on m), then the sum of the first nb_valid[b, t] books in the RECEIVER's order (ops.rvq_dequant_layers,
    what ResidualVQEMA.from_indices(nb_valid=) runs).  ``nb_valid``: uint8 [B, n] for the folded z[1, D, B*n].  Returns
    (q, idx); d q / d z = nb_valid[b, t] * I per token -- the reference STE's nb * I at the token's own book count, 0 for a lost
    token, which then trains the predictor alone.  books receive no gradient."""

    @staticmethod
    def forward(ctx, z, books, nb_valid):
        zd = z.detach()
        _, idx = ops.rvq_ema_forward(zd, books, None, return_indices=True)
        B, n = nb_valid.shape
        q = torch.empty_like(zd)                                              # token-folded [1, D, B*n]
        ops.rvq_dequant_layers(idx.reshape(books.shape[0], B, n), books, nb_valid, out=q, out_strides=(n, B * n))
        ctx.scale = nb_valid.reshape(1, 1, -1).to(zd.dtype)
        ctx.mark_non_differentiable(idx)
        return q, idx

    @staticmethod
    def backward(ctx, g, _gidx):
        return g * ctx.scale, None, None


def unfreeze_decoder(net, *, snake=True, bias=True):
    """Fine-tune the tactile decoder: set ``requires_grad`` on ``net.T_DEC``'s parameters (``net``: a model with a ``T_DEC``, or a
    dac.Decoder itself) and return them for the optimiser.  The conv weights (weight_g / weight_v) always; the Snake alphas and
    the conv biases unless switched off.  The constructors freeze T_DEC as the reference does; this is the opt-in that undoes it.
    ``forward_step`` then trains the decoder too: dac.Decoder.forward records the weight-gradient backward (backward_params)."""
    dec = getattr(net, "T_DEC", net)
    out = []
    for name, p in dec.named_parameters():
        kind = name.rsplit(".", 1)[-1]
        want = kind in ("weight_g", "weight_v") or (kind == "alpha" and snake) or (kind == "bias" and bias)
        p.requires_grad_(bool(want))
        if want:
            out.append(p)
    return out
