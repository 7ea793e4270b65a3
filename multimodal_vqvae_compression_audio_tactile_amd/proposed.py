"""The reference's own modules on the hot path, same names / constructor arguments / state-dict keys, running on
libmvq_hip.so:  PosEnc1D, TokenNorm, CrossPredictor, ResidualVQEMA, AllPredAR (forward), ProposedEval, ProposedWrapper.

Reference: Training/compare_dacvsproposal_5.py:214-326 (train-time classes) and
Evaluation/dac_vcpwq_proposed6_latency.py:339-487 (eval-time classes with ``n_books_use`` / ``encode_latents``).

MI355X-first differences that do not change results:
  * inside the AR loop every chunk tensor is kept TOKEN-FOLDED as [1, C, B*Tc] (column b*Tc+i), so the six
    predictor GEMMs, proj_down/up and the RVQ search see N = B*Tc contiguous columns instead of B tiny
    [C,16] problems; LayerNorm / attention take (batch, channel) strides for that layout;
  * PosEnc1D add is fused into the LayerNorm kernel, tanh and the clamp(scale) multiply into TokenNorm's,
    residual adds into GEMM epilogues;
  * the shift-by-one input ``zt_prev`` is built exactly as the reference does (only column 0 of a chunk with
    s > 0 is non-zero -- SURVEY.md section 3.1 "Observed data dependency").
Training (row f1 of SURVEY.md section 8): with autograd enabled, ``AllPredAR.forward_step`` builds the graph out of the
HIP-backed autograd Functions in train.py (same forward kernels, HIP backward kernels), so the reference's
``total.backward(); opt.step()`` works on these modules unchanged; ``net.train()`` enables the ctx dropout.
"""
from __future__ import annotations

import math
import os
from typing import Optional

import numpy as np
import torch
import torch.nn as nn

from . import ops, train
from ._lib import MvqError
from . import dac as _dac
from .dac import _Packed

CODE_DIM = 96        # Training/compare_dacvsproposal_5.py:68
AR_CHUNK_TOK = 16    # ...:65
EMA_DECAY = 0.99     # ...:69


class PosEnc1D(nn.Module):
    def __init__(self, c, max_len=8192):
        super().__init__()
        pe = torch.zeros(max_len, c)
        pos = torch.arange(0, max_len).unsqueeze(1)
        div = torch.exp(torch.arange(0, c, 2) * (-math.log(10000.0) / c))
        pe[:, 0::2] = torch.sin(pos * div)
        pe[:, 1::2] = torch.cos(pos * div)
        self.register_buffer("pe", pe)


class TokenNorm(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.ln = nn.LayerNorm(c)

    @torch.no_grad()
    def forward(self, z):
        return ops.layernorm_c(z, self.ln.weight.detach(), self.ln.bias.detach(), eps=self.ln.eps)


class _PackedLinear:
    """K-major packed image of an nn.Linear / 1x1 nn.Conv1d weight, rebuilt when the parameter changes."""

    def __init__(self, mod):
        self.mod = mod
        self.cache = _Packed()

    def wp(self):
        w = self.mod.weight
        return self.cache.get((w,), lambda: ops.pack_conv1d(w.detach().reshape(w.shape[0], w.shape[1], 1)))

    def wp_dgrad(self):
        """The input-gradient image of the same weight (train.Linear.backward), once per weight version instead of once per AR chunk."""
        w = self.mod.weight
        if not hasattr(self, "cache_d"):
            self.cache_d = _Packed()
        return self.cache_d.get((w,), lambda: ops.pack_conv1d_dgrad(w.detach().reshape(w.shape[0], w.shape[1], 1)))

    def __call__(self, x, residual=None, gelu=False):
        w = self.mod.weight
        b = self.mod.bias.detach() if getattr(self.mod, "bias", None) is not None else None
        if gelu and (w.shape[1] % 32 or w.shape[0] < 64):                  # GELU epilogue exists on the MFMA tiles only
            return ops.gelu(ops.conv1d(x, self.wp(), w.shape[0], 1, bias=b, residual=residual))
        return ops.conv1d(x, self.wp(), w.shape[0], 1, bias=b, residual=residual, gelu=gelu)


class CrossPredictor(nn.Module):
    def __init__(self, c, heads=8, mlp_mul=2, dropout=0.1):
        super().__init__()
        assert c % heads == 0
        self.pos = PosEnc1D(c)
        self.h, self.dh = heads, c // heads
        self.ln_q, self.ln_kv = nn.LayerNorm(c), nn.LayerNorm(c)
        self.q_proj, self.k_proj, self.v_proj = nn.Linear(c, c, False), nn.Linear(c, c, False), nn.Linear(c, c, False)
        self.out = nn.Linear(c, c, False)
        self.drop = nn.Dropout(dropout)
        self.ffn = nn.Sequential(nn.LayerNorm(c), nn.Linear(c, mlp_mul * c), nn.GELU(), nn.Linear(mlp_mul * c, c))
        self._lin = {n: _PackedLinear(m) for n, m in (("q", self.q_proj), ("k", self.k_proj), ("v", self.v_proj),
                                                      ("o", self.out), ("f1", self.ffn[1]), ("f3", self.ffn[3]))}

    @torch.no_grad()
    def keys_values(self, qa_folded, folded_batch, chunk):
        """K and V of EVERY chunk in one pass: the audio side of the predictor does not depend on the AR state, so the
        per-chunk LayerNorm + two GEMMs (15 launches per segment batch) collapse into 3 over all B*Ta tokens.  PosEnc1D
        restarts at each chunk (the reference applies it per chunk, Training/...5.py:305-309): row t of the table is
        pe[t mod chunk]."""
        Ta = qa_folded.shape[2] // folded_batch
        key = (Ta, chunk, str(qa_folded.device))
        if getattr(self, "_pe_tiled", (None,))[0] != key:
            reps = (Ta + chunk - 1) // chunk
            self._pe_tiled = (key, self.pos.pe[:chunk].repeat(reps, 1)[:Ta].contiguous())
        kv = ops.layernorm_c(qa_folded, self.ln_kv.weight.detach(), self.ln_kv.bias.detach(), pe=self._pe_tiled[1],
                             eps=self.ln_kv.eps, folded_batch=folded_batch)
        return self._lin["k"](kv), self._lin["v"](kv)

    def _chunk_kernels_fit(self, Q, K, fb, bwd=False):
        """The AR chunks (16 tokens) stay on the chunk attention kernels; only longer calls -- the PLC predictor over a whole
        latent sequence -- take the full-sequence ones."""
        n = fb or 1
        tq, tk = Q.shape[-1] // n, K.shape[-1] // n
        return ops.attention_fits(self.dh, tq, tk) and (not bwd or ops.attention_bwd_fits(self.dh, tq, tk))

    @torch.no_grad()
    def run(self, zt_prev, za, folded_batch=None, kv_all=None, kv_slice=None, attend=None, key_mask=None):
        """zt_prev[B,C,Tq], za[B,C,Tk] (or both token-folded [1,C,B*T] with folded_batch=B) -> same layout.
        kv_all = keys_values(...) with kv_slice = (s, tk): attend to columns [s, s+tk) of the precomputed K / V.
        attend: a callable Q -> ctx that does the attention itself (the receiver's chunk-as-batch calls).
        key_mask (uint8 [B, Tk] on the device, nonzero = key present; inference only): item b attends over its present keys
        alone, through the masked full-sequence kernel (bit-equal to the chunk kernel wherever that one fits)."""
        fb = folded_batch
        if key_mask is not None and (attend is not None or kv_all is not None):
            raise MvqError("CrossPredictor.run: key_mask goes with the plain call; attend / kv_all do their own attention")
        pe = self.pos.pe
        q = ops.layernorm_c(zt_prev, self.ln_q.weight.detach(), self.ln_q.bias.detach(), pe=pe, eps=self.ln_q.eps,
                            folded_batch=fb)
        L = self._lin
        if attend is not None:
            ctx = attend(L["q"](q))
        elif kv_all is not None:
            ctx = ops.attention_kv_slice(L["q"](q), kv_all[0], kv_all[1], self.h, fb, kv_slice[0], kv_slice[1])
        else:
            kv = ops.layernorm_c(za, self.ln_kv.weight.detach(), self.ln_kv.bias.detach(), pe=pe, eps=self.ln_kv.eps,
                                 folded_batch=fb)
            Q, K, V = L["q"](q), L["k"](kv), L["v"](kv)
            if key_mask is not None:
                ctx = ops.attention_seq(Q, K, V, self.h, folded_batch=fb, kmask=key_mask)
            else:
                attn = ops.attention if self._chunk_kernels_fit(Q, K, fb) else ops.attention_seq   # whole-sequence calls (PLC)
                ctx = attn(Q, K, V, self.h, folded_batch=fb)
        y1 = L["o"](ctx, residual=q)                                        # out(ctx) + q
        hdn = ops.layernorm_c(y1, self.ffn[0].weight.detach(), self.ffn[0].bias.detach(), eps=self.ffn[0].eps,
                              folded_batch=fb)
        hdn = L["f1"](hdn, gelu=True)                                       # nn.GELU() in the GEMM epilogue
        return L["f3"](hdn, residual=y1)                                    # ffn(y) + y

    def run_train(self, zt_prev, za, folded_batch, key_mask=None):
        """Same computation as run() on token-folded tensors, recorded for autograd (train.py Functions).
        key_mask (uint8 [B, Tk] on the device, nonzero = key present; not differentiated): item b attends over its present keys
        alone -- the masked chunk kernel and its backward where the shape fits them, else the masked full-sequence pair."""
        fb, pe, L = folded_batch, self.pos.pe, self._lin
        if key_mask is not None and za.shape[-1] == 0:
            key_mask = None                                                     # no key to mask
        lin = lambda n, mod, x, res=None: train.Linear.apply(x, mod.weight, getattr(mod, "bias", None), res, L[n])
        q = train.LayerNormC.apply(zt_prev, self.ln_q.weight, self.ln_q.bias, pe, self.ln_q.eps, fb)
        kv = train.LayerNormC.apply(za, self.ln_kv.weight, self.ln_kv.bias, pe, self.ln_kv.eps, fb)
        Q, K, V = lin("q", self.q_proj, q), lin("k", self.k_proj, kv), lin("v", self.v_proj, kv)
        attn = train.Attention if self._chunk_kernels_fit(Q, K, fb, bwd=True) else train.AttentionSeq
        ctx = attn.apply(Q, K, V, self.h, fb) if key_mask is None else attn.apply(Q, K, V, self.h, fb, key_mask)
        if self.training and self.drop.p > 0:
            ctx = train.Dropout.apply(ctx, float(self.drop.p))
        y1 = lin("o", self.out, ctx, q)
        hdn = train.LayerNormC.apply(y1, self.ffn[0].weight, self.ffn[0].bias, None, self.ffn[0].eps, fb)
        hdn = train.Gelu.apply(lin("f1", self.ffn[1], hdn))
        return lin("f3", self.ffn[3], hdn, y1)

    def forward(self, zt_prev, za, key_mask=None):
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            if key_mask is not None:
                raise MvqError("CrossPredictor: key_mask is inference only (no backward under a key mask); use torch.no_grad()")
            B, C, Tq = zt_prev.shape
            fold = lambda x: x.permute(1, 0, 2).reshape(1, C, -1).contiguous()
            y = self.run_train(fold(zt_prev), fold(za), B)
            return y.reshape(C, B, Tq).permute(1, 0, 2).contiguous()
        if self.training and self.drop.p > 0:
            raise MvqError("CrossPredictor: train-mode dropout needs autograd enabled; call .eval() for inference")
        return self.run(zt_prev, za, key_mask=key_mask)


class ResidualVQEMA(nn.Module):
    """Residual VQ with EMA codebooks.  ``forward(z[B,D,T], n_books_use=None)``; ``ema_step(z_tokens)``."""

    def __init__(self, dim: int, n_books: int, n_embed: int, decay: float = EMA_DECAY):
        super().__init__()
        self.books = nn.ParameterList([nn.Parameter(torch.randn(n_embed, dim) / math.sqrt(dim))
                                       for _ in range(n_books)])
        self.decay = float(decay)
        self.n_books, self.n_embed = int(n_books), int(n_embed)
        self.dim = int(dim)
        self._stack = _Packed()

    def stacked(self) -> torch.Tensor:
        """[n_books, K, D] view for the kernel.  Re-stacked on every call (1.5 MB at most): the reference updates the
        books through ``.data`` (ema_step), which no version counter sees, so nothing derived from them is cached."""
        return torch.stack([b.detach().float() for b in self.books]).contiguous()

    @torch.no_grad()
    def forward(self, z, n_books_use: Optional[int] = None, return_indices: bool = False):
        if len(self.books) == 0:
            return torch.zeros_like(z)
        return ops.rvq_ema_forward(z, self.stacked(), n_books_use, return_indices=return_indices)

    @torch.no_grad()
    def from_indices(self, idx, n_books_use: Optional[int] = None, out=None, out_strides=None, nb_valid=None):
        """The receiver's dequantisation: idx[nb, B, T] -> qD[B, D, T] = ((+0 + e_0[idx_0]) + e_1[idx_1]) + ... over the first
        min(nb, n_books_use) books.  (The forward's straight-through sum needs the encoder-side residual: round-off apart.)
        ``nb_valid`` (uint8 [B, T] on the device): token (b, t) sums only its first nb_valid[b, t] of those books -- what arrived
        over a lossy channel; 0 gives a zero vector."""
        if len(self.books) == 0:
            if out is None:
                return torch.zeros(idx.shape[1], self.dim, idx.shape[2], device=idx.device)
            return out.zero_()
        if nb_valid is not None:
            return ops.rvq_dequant_layers(idx.to(self.books[0].device), self.stacked(), nb_valid, n_books_use, out=out,
                                          out_strides=out_strides)
        return ops.rvq_dequant(idx.to(self.books[0].device), self.stacked(), n_books_use, out=out, out_strides=out_strides)

    @torch.no_grad()
    def ema_step(self, z_tokens):
        books = self.stacked()
        ops.rvq_ema_step_(z_tokens, books, self.decay)
        for i, p in enumerate(self.books):
            p.data.copy_(books[i])


class _ProposedBase(nn.Module):
    def __init__(self, A_ENC, A_QUANT, T_ENC, T_DEC, c_lat, rvq_books, rvq_embed, decay=EMA_DECAY):
        super().__init__()
        self.A_ENC, self.A_QUANT, self.T_ENC, self.T_DEC = A_ENC, A_QUANT, T_ENC, T_DEC
        for m in [self.A_ENC, self.A_QUANT, self.T_ENC, self.T_DEC]:
            if m is not None:
                for p in m.parameters():
                    p.requires_grad_(False)
        self.predict = CrossPredictor(c=c_lat, heads=8, mlp_mul=2, dropout=0.1)
        self.tokennorm = TokenNorm(c_lat)
        self.scale = nn.Parameter(torch.tensor(0.08))
        self.proj_down = nn.Conv1d(c_lat, CODE_DIM, 1)
        self.proj_up = nn.Conv1d(CODE_DIM, c_lat, 1)
        self.vq = ResidualVQEMA(dim=CODE_DIM, n_books=rvq_books, n_embed=rvq_embed, decay=decay)
        self._pd, self._pu = _PackedLinear(self.proj_down), _PackedLinear(self.proj_up)
        self._scale_host = None

    def _scale_raw(self) -> float:
        """The scale parameter as a host float (one device read, cached per parameter version)."""
        key = (self.scale._version, self.scale.data_ptr())
        if self._scale_host is None or self._scale_host[0] != key:
            self._scale_host = (key, float(self.scale.detach().float().item()))
        return self._scale_host[1]

    def _scale_value(self) -> float:
        """clamp(scale, 5e-3, 0.5)   (Training/compare_dacvsproposal_5.py:314)."""
        return min(max(self._scale_raw(), 5e-3), 0.5)

    def _rate_books(self, books_use):
        """The books in use: StreamInfo.nb of what compress_packets sends."""
        n_books = len(self.vq.books)
        return n_books if books_use is None else max(0, min(int(books_use), n_books))

    def _rate_resolve(self, rate, books_use, packet_tok):
        """The refusals of sender rate control, before any launch -> (packet_tok, (min_books, mode, tol2, budget))."""
        from . import packets
        if not isinstance(rate, packets.Rate):
            raise ValueError(f"rate must be a packets.Rate, not {type(rate).__name__}")
        if ops.get_arith() != "f32":
            raise ValueError(f"rate control claims bit-equality with the receiver; arithmetic mode {ops.get_arith()!r} makes no "
                             "parity claim")
        packet_tok = packets.PACKET_TOK if packet_tok is None else int(packet_tok)
        n_books = len(self.vq.books)
        nb_use = n_books if books_use is None else max(0, min(int(books_use), n_books))
        return packet_tok, rate.resolve(nb_use, packet_tok, AR_CHUNK_TOK)

    def _audio_rate_resolve(self, audio_rate, audio_books, packet_tok):
        """The refusals of audio rate control, before any launch -> (audio_rate, na_use, packet_tok)."""
        from . import packets
        audio_rate = packets.Rate() if audio_rate is None else audio_rate
        if not isinstance(audio_rate, packets.Rate):
            raise ValueError(f"audio_rate must be a packets.Rate, not {type(audio_rate).__name__}")
        if ops.get_arith() != "f32":
            raise ValueError(f"audio rate control claims bit-equality with the receiver; arithmetic mode {ops.get_arith()!r} makes no "
                             "parity claim")
        stages = self.A_QUANT.n_codebooks
        if audio_books is None:
            na_use = stages
        else:
            if isinstance(audio_books, bool) or int(audio_books) != audio_books or not 1 <= int(audio_books) <= stages:
                raise ValueError(f"audio_books = {audio_books!r} outside 1..{stages} (the quantiser's stages)")
            na_use = int(audio_books)
        packet_tok = packets.PACKET_TOK if packet_tok is None else int(packet_tok)
        audio_rate.resolve(na_use, packet_tok, AR_CHUNK_TOK)
        if audio_rate.beam != 1:
            raise ValueError(f"audio_rate: beam = {audio_rate.beam} -- the audio quantiser's search has no beam (rate= takes one)")
        return audio_rate, na_use, packet_tok

    def _fec_resolve(self, fec, K, nb, packet_tok, what="fec"):
        """The refusals of forward error correction, before any launch (packets.Fec.resolve against the 16-token chunk: a parity
        group never straddles a chunk, which is what lets a streaming session emit the whole-item parity chunk by chunk)."""
        from . import packets
        if not isinstance(fec, packets.Fec):
            raise ValueError(f"{what} must be a packets.Fec, not {type(fec).__name__}")
        if ops.get_arith() != "f32":
            raise ValueError(f"{what}: forward error correction claims bit-equality with the whole-item and streaming paths; arithmetic "
                             f"mode {ops.get_arith()!r} makes no parity claim")
        packet_tok = packets.PACKET_TOK if packet_tok is None else int(packet_tok)
        fec.resolve(packets.StreamInfo(int(K), int(nb), AR_CHUNK_TOK, packet_tok), chunk_tok=AR_CHUNK_TOK)
        return fec

    @staticmethod
    def _fec_packets(fec, fec_packets, B, who, what="fec"):
        """The parity packets of a whole-item call, per item -> ``fec_packets``, or B times None for a stream without a Fec."""
        if fec is None:
            return [None] * B
        if fec_packets is None or len(fec_packets) != B:
            raise MvqError(f"{who}: {what}= needs {what}_packets, one list of parity packets per item (empty when none arrived)")
        return fec_packets

    @staticmethod
    def _rx_host(front, B, T, *per_item):
        """Host: the whole-item upload of ``B`` items through the front end (stream._RxFront, which owns its format): gather_item
        and fill per item; ``per_item`` = the tactile, audio, parity and audio parity packets, each a list per item -> (lay, host)."""
        lay = front.layout(B, T)
        host = np.empty(lay.size, np.uint8)
        for b in range(B):
            front.fill(host, lay, b, front.gather_item(*(pk[b] for pk in per_item), T))
        return lay, host

    @torch.no_grad()
    def _ar_latents(self, qa, zt, books_use=None, want_tokens=False, tactile_only=False, want_indices=False, z_prev=None,
                    z_last_out=None, rate=None, packet_tok=None):
        """The chunked AR loop (Training/...5.py:302-320 == Evaluation/...6_latency.py:461-477).
        ``want_indices``: also return the per-book code indices idx[n_books_use, B, Tlat] (int64).

        Streaming (stream.StreamSender): a chunk depends on the ones before it through z_run[..., s-1] alone, so a sequence is
        quantised piece by piece, each piece a whole number of 16-token chunks (the last may be shorter): ``z_prev`` ([B, C]
        contiguous fp32 on the device) is the last z_run token of the piece before and becomes column 0 of the first chunk's
        zt_prev; ``z_last_out`` (same shape; may be the z_prev buffer) receives this piece's last z_run token.  Both None:
        today's launch sequence exactly.  The opt-in persistent kernel carries no token: such a call takes the staged form or the
        Python loop.

        ``rate`` (a packets.Rate; packets of ``packet_tok`` tokens, default packets.PACKET_TOK): closed-loop sender rate control.
        After each chunk's search one ops.rvq_rate launch decides on the device how many books each packet carries and replaces the
        straight-through qD by the sum the receiver will form from exactly those books, so z_run -- and through z_run[..., s-1]
        every later chunk -- is what decode_latents(nb_valid=) reconstructs, bit for bit (given ``qa`` from the codes).  Implies
        ``want_indices`` and returns (z_run, r_tokens, idx, nb_valid uint8 [B, Tlat], nb_sent uint8 [B, P]).  Only in "f32"
        arithmetic; the persistent kernel is never taken.  None: today's launches exactly.  ``rate.beam`` > 1 (DESIGN.md section
        33): each chunk's search is ops.rvq_beam -- the path with the smallest final residual among ``beam`` per token -- in place
        of the greedy one; the rate launch reads its indices as it reads the greedy ones, so z_run stays the receiver's.  1:
        today's launches exactly."""
        B, C, Tlat = zt.shape
        rate_args, beam = None, 1
        if rate is not None:
            packet_tok, rate_args = self._rate_resolve(rate, books_use, packet_tok)
            want_indices = True
            beam = int(rate.beam)
        carried = z_prev is not None or z_last_out is not None
        if carried:
            if tactile_only:
                raise MvqError("_ar_latents: z_prev / z_last_out carry the recursion; tactile_only has none")
            for t, name in ((z_prev, "z_prev"), (z_last_out, "z_last_out")):
                if t is not None and not (isinstance(t, torch.Tensor) and t.device == zt.device and t.dtype == torch.float32
                                          and tuple(t.shape) == (B, C) and t.is_contiguous()):
                    raise MvqError(f"_ar_latents: {name} must be a contiguous fp32 tensor [B={B}, C={C}] on {zt.device}")
        z_run = torch.zeros_like(zt)
        r_tokens = torch.empty(B, CODE_DIM, Tlat, device=zt.device, dtype=torch.float32) if want_tokens else None
        idx_all = [] if want_indices else None
        if B == 0 or Tlat == 0:                                               # empty batch / clip shorter than a token
            if rate is not None:
                return (z_run, r_tokens, torch.zeros(0, B, Tlat, dtype=torch.int64, device=zt.device),
                        torch.zeros(B, Tlat, dtype=torch.uint8, device=zt.device), torch.zeros(B, 0, dtype=torch.uint8, device=zt.device))
            return (z_run, r_tokens, torch.zeros(0, B, Tlat, dtype=torch.int64, device=zt.device)) if want_indices \
                else (z_run, r_tokens)
        nb_valid = nb_sent = None
        if rate is not None:                                                  # the rate kernel writes every element (no books: zeros)
            mk = torch.empty if len(self.vq.books) else torch.zeros
            nb_valid = mk(B, Tlat, dtype=torch.uint8, device=zt.device)
            nb_sent = mk(B, (Tlat + packet_tok - 1) // packet_tok, dtype=torch.uint8, device=zt.device)
        scale = self._scale_value()
        ln = self.tokennorm.ln
        books = self.vq.stacked() if len(self.vq.books) else None             # ONE stack per call, not one per chunk
        kv_all = None
        if not tactile_only:
            Ta = min(qa.shape[-1], Tlat)                                      # audio may be shorter (whole-file mode)
            if Ta > 0:                                                        # K, V of all chunks up front (3 launches)
                kv_all = self.predict.keys_values(ops.fold_time_slice(qa, 0, Ta), B, AR_CHUNK_TOK)
        mode = self._ar_one_call_mode(zt, books)
        if rate is not None and books is None:
            mode = None                                                       # no books: nothing to search or rate; the loop below writes zeros
        if mode == "fused" and (carried or rate is not None):
            mode = "staged" if zt.shape[0] <= self.AR_STAGED_MAX_BATCH and self._ar_shapes_covered(zt, books) else None
        if mode is not None:
            return self._ar_latents_fused(zt, z_run, r_tokens, kv_all, 0 if tactile_only else min(qa.shape[-1], Tlat), books, books_use,
                                          tactile_only, want_indices, staged=(mode == "staged"), z_prev=z_prev, z_last_out=z_last_out,
                                          rate=None if rate is None else (packet_tok,) + rate_args + (nb_valid, nb_sent), beam=beam)
        zt_prev, zp_n = None, -1      # the shift-by-one input: all zero except column 0 of each item (s > 0), so one zeroed
        for s in range(0, Tlat, AR_CHUNK_TOK):                               # buffer per chunk width serves every chunk
            e = min(Tlat, s + AR_CHUNK_TOK)
            n = e - s
            zt_c = ops.fold_time_slice(zt, s, e)                             # [1,C,B*n]
            if tactile_only:
                z_pred = None
            else:
                if n != zp_n:
                    zt_prev, zp_n = torch.zeros(1, C, B * n, device=zt.device, dtype=torch.float32), n
                if s > 0:                                                     # column 0 <- z_run[..., s-1]
                    ops.fold_column_into_(zt_prev, 0, z_run, s - 1, B)
                elif z_prev is not None:                                      # ... of the piece before
                    ops.copy_strided_(zt_prev, 0, (n, B * n), z_prev, 0, (C, 1), B, C, 1)
                ka = min(qa.shape[-1], e) - min(qa.shape[-1], s)
                if ka > 0:
                    z_pred = self.predict.run(zt_prev, None, folded_batch=B, kv_all=kv_all, kv_slice=(s, ka))
                else:
                    z_pred = self.predict.run(zt_prev, torch.zeros(1, C, 0, device=zt.device), folded_batch=B)
            rN = ops.layernorm_c(zt_c, ln.weight.detach(), ln.bias.detach(), eps=ln.eps, do_tanh=True, post_scale=scale,
                                 folded_batch=B, sub=z_pred)                  # tanh(TokenNorm(zt - z_pred)) * scale
            rD = self._pd(rN)                                                 # [1,96,B*n]
            if books is None:
                qD = torch.zeros_like(rD)
            elif rate is not None:      # the search's int32 indices go to the rate kernel as they are: the receiver's sum over the books sent
                if beam > 1:
                    idx = ops.rvq_beam(rD, books, beam, books_use, folded_batch=B)
                else:
                    _, idx = ops.rvq_ema_forward(rD, books, books_use, return_indices="int32")
                idx_all.append(idx.reshape(idx.shape[0], B, n))
                qD = ops.rvq_rate(rD, idx, books, rate, packet_tok, books_use, folded_batch=B, nb_valid_out=nb_valid,
                                  nb_sent_out=nb_sent, col=s)[0]
            elif want_indices:
                qD, idx = ops.rvq_ema_forward(rD, books, books_use, return_indices=True)
                idx_all.append(idx.reshape(idx.shape[0], B, n))
            else:
                qD = ops.rvq_ema_forward(rD, books, books_use)
            z_hat = self._pu(qD, residual=z_pred)
            ops.unfold_into_(z_run, s, z_hat, B)
            if want_tokens:
                ops.unfold_into_(r_tokens, s, rD, B)
        if z_last_out is not None:
            ops.copy_strided_(z_last_out, 0, (C, 1), z_run, Tlat - 1, (C * Tlat, Tlat), B, C, 1)
        if want_indices:
            idx = torch.cat(idx_all, dim=2).long() if idx_all else torch.zeros(0, B, Tlat, dtype=torch.int64)
            return (z_run, r_tokens, idx) if rate is None else (z_run, r_tokens, idx, nb_valid, nb_sent)
        return z_run, r_tokens

    # The loop as ONE persistent kernel (csrc/ar_fused.hip: eleven stages per chunk between grid-wide barriers), for up to this many
    # segments.  OFF by default (0): measured at the reference's operating points (tools/ar_fused_ab.py, gpurun_out/f8) it is bit-equal
    # to the launch-per-stage loop and SLOWER -- 1.22 against 0.99 ms for one segment, 1.74 against 1.09 ms for six.  The stages are
    # 5-45 us of dependent chain each; at that length the command processor already has the next launch queued behind the running
    # kernel, so a launch boundary costs less than the ~4 us a grid barrier (a device-scope atomic, an L2 write-back and an
    # invalidate across eight XCDs) does.  Kept as an opt-in (MVQ_AR_FUSED_MAX_BATCH) with its parity tests.
    AR_FUSED_MAX_BATCH = int(_dac.HOST_ENV_SEEN.get("MVQ_AR_FUSED_MAX_BATCH", "0"))

    # The loop as ONE HOST CALL of the same stand-alone launches (mvq_ar_latents_staged_f32), for up to this many segments: at one
    # segment the Python loop's ~85 foreign calls and their allocations cost as much host time as the kernels take on the device
    # (eager encode 2.5 ms against 2.3 replayed as a graph).  Needs every GEMM in the latency form's range: 8 segments at most.
    AR_STAGED_MAX_BATCH = min(8, int(_dac.HOST_ENV_SEEN.get("MVQ_AR_STAGED_MAX_BATCH", "8")))

    def _ar_shapes_covered(self, zt, books):
        p = self.predict
        return (zt.is_cuda and zt.shape[0] > 0 and ops.get_arith() == "f32"
                and zt.shape[1] == 1024 and p.h == 8 and p.ffn[1].out_features == 2048 and CODE_DIM == 96 and p.ln_q.eps == p.ffn[0].eps
                and (books is None or (books.shape[1] <= 512 and books.shape[2] == CODE_DIM)))

    def _ar_one_call_mode(self, zt, books):
        """"fused" (opt-in persistent kernel), "staged" (one host call, stand-alone launches) or None (the Python loop)."""
        if self._ar_fused_wanted(zt, books):
            return "fused"
        if zt.shape[0] <= self.AR_STAGED_MAX_BATCH and self._ar_shapes_covered(zt, books):
            return "staged"
        return None

    def _ar_fused_wanted(self, zt, books):
        p = self.predict
        return (zt.is_cuda and 0 < zt.shape[0] <= self.AR_FUSED_MAX_BATCH and ops.get_arith() == "f32"
                and not torch.cuda.is_current_stream_capturing()            # a cooperative launch is not capturable
                and zt.shape[1] == 1024 and p.h == 8 and p.ffn[1].out_features == 2048 and CODE_DIM == 96 and p.ln_q.eps == p.ffn[0].eps
                and (books is None or (books.shape[1] <= 512 and books.shape[2] == CODE_DIM)))

    def _ar_latents_fused(self, zt, z_run, r_tokens, kv_all, t_audio, books, books_use, tactile_only, want_indices, staged=False,
                          z_prev=None, z_last_out=None, rate=None, beam=1):
        B, _, Tlat = zt.shape
        p, L, ln = self.predict, self.predict._lin, self.tokennorm.ln
        nb = 0 if books is None else (books.shape[0] if books_use is None else max(0, min(int(books_use), books.shape[0])))
        idx = torch.empty(nb, B, Tlat, device=zt.device, dtype=torch.int32) if want_indices else None
        det = lambda t: None if t is None else t.detach()
        ops.ar_latents_fused(
            zt.contiguous(), z_run, k_all=None if kv_all is None else kv_all[0], v_all=None if kv_all is None else kv_all[1],
            t_audio=t_audio if kv_all is not None else 0, pe=p.pos.pe, ln_q=(det(p.ln_q.weight), det(p.ln_q.bias)),
            wq=L["q"].wp(), wo=L["o"].wp(), ln_f=(det(p.ffn[0].weight), det(p.ffn[0].bias)), w1=L["f1"].wp(), b1=det(p.ffn[1].bias),
            w3=L["f3"].wp(), b3=det(p.ffn[3].bias), ln_eps=p.ln_q.eps, tok=(det(ln.weight), det(ln.bias)), tok_eps=ln.eps,
            scale=self._scale_value(), wd=self._pd.wp(), bd=det(self.proj_down.bias), wu=self._pu.wp(), bu=det(self.proj_up.bias),
            books=books, books_use=books_use, heads=p.h, c_ff=p.ffn[1].out_features, code_dim=CODE_DIM, r_tokens=r_tokens, idx_out=idx,
            tactile_only=tactile_only, chunk=AR_CHUNK_TOK, staged=staged, z_prev=z_prev, z_last_out=z_last_out, rate=rate, beam=beam)
        if rate is not None:
            return z_run, r_tokens, idx.long(), rate[5], rate[6]
        if want_indices:
            return z_run, r_tokens, idx.long()
        return z_run, r_tokens

    # The two encoder branches (qa = A_QUANT(A_ENC(a)), zt = T_ENC(t)) are independent; up to this many segments they run on two
    # HIP streams (round 1: 8 % at B = 1-8, 5 % at 32, 1 % at 48-64).  At 256 segments two streams still give 330.6 -> 329.7 ms
    # per step (the under-filled tail / latent-rate launches of one branch overlap the other's; gpurun_out/r3l, twice on one
    # box), but concurrent kernels stretch each other's durations, so the per-kernel HIP-event / rocprofv3 figures the bench
    # reports (roofline of the dominant kernel) would no longer describe a kernel running alone.  The default therefore keeps
    # one stream at throughput batch sizes; MVQ_TWO_STREAM_MAX_BATCH raises the cap.
    TWO_STREAM_MAX_BATCH = int(_dac.HOST_ENV_SEEN.get("MVQ_TWO_STREAM_MAX_BATCH", "64"))      # read once at import, reported by plan_overrides()

    def _two_streams(self, x, audio_branch, tactile_branch):
        """THE rule for the two encoder branches, which are independent: ``audio_branch()`` -> a tuple of tensors,
        ``tactile_branch()`` -> zt; -> (that tuple, zt).  In the latency regime (few segments ``x.shape[0]``: every launch underfills
        the 256 CUs) the audio branch runs on a second HIP stream beside the tactile branch and everything it returned is recorded
        on the current stream; otherwise the audio branch, then the tactile one, on the current stream."""
        # The opt-in arithmetic modes (frozen, non-parity) keep ONE stream: round 5 saw the audio branch of the FIRST two-stream call
        # of a fresh model come back wrong in bf16x6 (B = 2, fixture G4) in 4 of 4 plain runs and in 0 of 12 runs with any
        # perturbation (a synchronisation, NaN-poisoned allocations, one more reference held, any single new kernel switched off);
        # the cause was not established, the exact path has never shown it.
        if x.shape[0] > self.TWO_STREAM_MAX_BATCH or not x.is_cuda or ops.get_arith() != "f32":
            audio = audio_branch()
            return audio, tactile_branch()
        cur = torch.cuda.current_stream()
        side = getattr(self, "_side_stream", None)
        if side is None or side.device != x.device:
            side = torch.cuda.Stream(device=x.device)
            self._side_stream = side
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            audio = audio_branch()
        zt = tactile_branch()
        cur.wait_stream(side)
        for t in audio:
            t.record_stream(cur)
        return audio, zt

    def _encode_branches(self, a_1T, t_1T):
        """qa = A_QUANT(A_ENC(a)) and zt = T_ENC(t), on one or two HIP streams (``_two_streams``)."""
        def audio():
            za = self.A_ENC(a_1T)
            qa, *_ = self.A_QUANT(za)
            return za, qa
        (_, qa), zt = self._two_streams(a_1T, audio, lambda: self.T_ENC(t_1T))
        return qa, zt

    @torch.no_grad()
    def encode_latents_with_indices(self, a_1T, t_1T, books_use=None, rate=None, packet_tok=None, audio_books=None, audio_rate=None):
        """encode_latents plus what a transmitter would send: -> (z_run, audio codes[B,32,Ta] of A_QUANT, RVQ idx[n_books_use,B,Tlat]).

        ``rate`` (packets.Rate; packets of ``packet_tok`` tokens, default packets.PACKET_TOK): closed-loop sender rate control
        (_ar_latents) -> (z_run, codes, idx, nb_sent uint8 [B, P]): packet p of item b carries the first nb_sent[b, p] books of
        its tokens' rows of idx, and z_run is bit for bit what decode_latents(codes, idx, nb_valid=<nb_sent per token>) gives: the
        loop runs on the books sent and on qa = A_QUANT.from_codes(codes), the receiver's audio latent, not the straight-through
        one.

        ``audio_books`` (1..32: the stages of A_QUANT the audio stream carries, default all) / ``audio_rate`` (packets.Rate, default
        Rate(): every packet carries ``audio_books`` stages): the audio codes travel in layered packets too.  When either is
        given the loop runs closed on BOTH streams (``rate`` None is Rate()): ops.dac_rvq_rate decides on the device how many stages
        each audio packet carries and forms qa from exactly those, and the AR loop runs on that qa.
        -> (z_run, codes, idx, nb_sent uint8 [B, P], na_sent uint8 [B, Pa]): audio packet p of item b carries the first
        na_sent[b, p] rows of its tokens' columns of codes (all 32 rows are returned as A_QUANT made them), and z_run is bit for bit
        decode_latents(codes, idx, nb_valid=<nb_sent per token>, na_valid=<na_sent per token>)."""
        audio = audio_books is not None or audio_rate is not None
        if audio:
            from . import packets
            audio_rate, na_use, packet_tok = self._audio_rate_resolve(audio_rate, audio_books, packet_tok)
            rate = packets.Rate() if rate is None else rate
        if rate is not None:
            self._rate_resolve(rate, books_use, packet_tok)                   # refusals before any launch
        za = self.A_ENC(a_1T)
        qa, codes, *_ = self.A_QUANT(za)
        if audio:
            qa_rx, _, na_sent = self.A_QUANT.rate(za, codes, audio_rate, packet_tok, na_use)
            z_run, _, idx, _, nb_sent = self._ar_latents(qa_rx, self.T_ENC(t_1T), books_use, rate=rate, packet_tok=packet_tok)
            return z_run, codes, idx, nb_sent, na_sent
        if rate is not None:
            z_run, _, idx, _, nb_sent = self._ar_latents(self.A_QUANT.from_codes(codes)[0], self.T_ENC(t_1T), books_use, rate=rate,
                                                         packet_tok=packet_tok)
            return z_run, codes, idx, nb_sent
        z_run, _, idx = self._ar_latents(qa, self.T_ENC(t_1T), books_use, want_indices=True)
        return z_run, codes, idx

    # ------------------------------------------------------------------------------------------------------------- receiver
    @torch.no_grad()
    def decode_latents(self, audio_codes=None, idx=None, *, qa=None, books_use=None, tactile_only=False, nb_valid=None,
                       conceal="predict", plc=None, z_prev=None, z_last_out=None, na_valid=None, audio_conceal="zero", qa_prev=None,
                       qa_last_out=None, qa_slots=None, qa_slots_dev=None, return_qa=False):
        """The receiver: z_run from what encode_latents_with_indices transmits -- audio codes[B,32,Ta] (int) and the RVQ
        indices idx[nb,B,Tlat] (int) -- or from ``qa`` directly instead of the codes.  The transmitter's loop without T_ENC,
        TokenNorm, proj_down and the search: z_hat = proj_up(qD) + z_pred, qD = the summed code vectors (from_indices),
        qa = A_QUANT.from_codes(codes).  Round-off apart it equals the transmitter's z_run (the quantisers' straight-through
        sums need encoder-side values the receiver does not have).

        z_pred depends on the loop only through column 0 of chunks s > 0 (z_run[s-1], the LAST token of the chunk before,
        which itself does not depend on the loop), so the receiver is two dependent passes instead of one pass per chunk
        (_rx_two_pass); the result is bit-equal to the per-chunk loop.

        Lossy channel: ``nb_valid`` ([B, T_lat] uint8 on the device: the books of each token that arrived; bool: all or none;
        None = all, today's path).  A token sums only the books it has (qD over the first nb_valid[b, t] books); a token with
        none is LOST and takes the audio-driven prediction uncorrected, z_hat = proj_up(0) + z_pred.  The recursion always runs
        on those values; loss changes qD alone, so the two passes stay valid.  ``conceal`` is a post-pass over that z_run:
        "predict" none; "zero" lost tokens become 0 (the unconcealed baseline AllPredPLC feeds its predictor); "plc"
        where(lost, plc.predict(z_run * ~lost, qa), z_run) with ``plc`` an AllPredPLC.  The mask is never read on the host: the
        launch sequence depends on shapes and ``conceal`` only, so a captured graph replays with another loss pattern written
        into the same nb_valid buffer.

        Lossy AUDIO stream: ``na_valid`` ([B, Ta] uint8 on the device: the stages of each audio token that arrived; bool: all or
        none; None = all, today's path launch for launch).  qa = A_QUANT.from_codes(codes, nq_valid=na_valid): a token sums only
        the stages it has, and an audio token of which NOTHING arrived is +0 in every channel -- the predictor attends over it as it
        would over silence.  That is the unconcealed baseline, ``audio_conceal="zero"``.
        ``conceal`` acts on the tactile tokens only; "plc" is handed the same qa.  Needs ``audio_codes`` (not ``qa``); never read
        on the host.

        ``audio_conceal`` acts on the audio tokens with na_valid == 0 (a token with at least one stage is a valid lower-rate token
        in every mode).  "mask": a lost audio token is not a key -- the predictor's softmax and value sum run over the arrived keys
        of the chunk, in ascending order, as if the lost columns were absent (mvq_attention_masked_f32; a chunk with none gives
        ctx = 0, as ka = 0 does).  "hold": a lost token takes the latent qa of the most recent arrived token of its item, across
        chunk borders, +0 before the first arrival (ops.hold_fill_ on qa right after from_codes), and then goes through ln_kv with
        its own position as any token does.  ``qa_prev`` / ``qa_last_out`` ([B, C] fp32 on the device; may be one buffer) carry the
        last held token between the pieces of a sequence, as z_prev / z_last_out carry the recursion; they belong to "hold".
        ``qa_slots`` (host integers, one per item; ``qa_slots_dev`` their int32 device copy): the items are sessions of a pool and
        qa_prev / qa_last_out are ONE buffer, the pool's [S, C] -- item b's held token is row qa_slots[b] of it
        (ops.hold_fill_(slots=); stream.StreamReceiverPoolAV).
        conceal="plc" is handed what the predictor saw: the held qa, or qa with the key mask.  With na_valid=None every token
        arrived and every mode is "zero".  The launch sequence depends on shapes and modes only.

        Streaming (stream.py): a chunk depends on the ones before it through z_run[..., s-1] alone, so a sequence is decoded
        piece by piece, each piece a whole number of 16-token chunks (the last may be shorter), with ``z_prev`` ([B, C] fp32 on the
        device) = the LAST token of the piece before, as the recursion saw it; pass 2 then feeds it to chunk 0 where it feeds zero
        today.  ``z_last_out`` ([B, C] fp32 on the device; may be the z_prev buffer itself) receives this piece's last token
        BEFORE the ``conceal`` post-pass, which is what the next piece's z_prev must be ("zero" would otherwise erase a lost
        last token that the whole-item recursion still reads).  Not with conceal="plc" (its predictor attends over the whole
        sequence) and not with tactile_only (no recursion to carry).  Both None: today's launch sequence exactly.

        ``return_qa``: -> (z_run, qa), qa [B, C, Ta] the audio latent AS THE PREDICTOR SAW IT -- under "hold" the held token at a lost
        one, under "zero" and "mask" +0 there (from_codes(nq_valid=) writes +0 and "mask" leaves it) -- which is what the
        receiver's audio decoder is fed (decode_av).  Not with tactile_only; no extra launch."""
        if idx is None:
            raise MvqError("decode_latents: idx (the RVQ indices [n_books, B, T_lat]) is required")
        dev = self.proj_up.weight.device
        idx = torch.as_tensor(idx).to(dev)
        if idx.dim() != 3:
            raise MvqError(f"decode_latents: idx must be [n_books, B, T_lat], got {tuple(idx.shape)}")
        _, B, Tlat = idx.shape
        C = self.proj_up.out_channels
        if conceal not in ("predict", "zero", "plc"):
            raise MvqError(f"decode_latents: conceal must be 'predict', 'zero' or 'plc', not {conceal!r}")
        if conceal == "plc":
            if tactile_only:
                raise MvqError("decode_latents: conceal='plc' predicts from the audio: not with tactile_only")
            if plc is None or not hasattr(plc, "predict"):
                raise MvqError("decode_latents: conceal='plc' needs plc (an AllPredPLC)")
            if Tlat > ops.ATTN_SEQ_MAX_T:
                raise MvqError(f"decode_latents: conceal='plc' at T_lat={Tlat} exceeds attention_seq's {ops.ATTN_SEQ_MAX_T} tokens")
        if z_prev is not None or z_last_out is not None:
            if conceal == "plc":
                raise MvqError("decode_latents: z_prev / z_last_out decode a piece of a sequence; conceal='plc' attends over the whole of it")
            if tactile_only:
                raise MvqError("decode_latents: z_prev / z_last_out carry the recursion; tactile_only has none")
            for t, name in ((z_prev, "z_prev"), (z_last_out, "z_last_out")):
                if t is not None and not (isinstance(t, torch.Tensor) and t.device == dev and t.dtype == torch.float32
                                          and tuple(t.shape) == (B, C) and t.is_contiguous()):
                    raise MvqError(f"decode_latents: {name} must be a contiguous fp32 tensor [B={B}, C={C}] on {dev}")
        if return_qa and tactile_only:
            raise MvqError("decode_latents: return_qa hands back the audio latent; tactile_only has none")
        if nb_valid is None:
            conceal = "predict"                                               # every token arrived whole: nothing to conceal
        else:
            if not isinstance(nb_valid, torch.Tensor) or nb_valid.dtype not in (torch.uint8, torch.bool):
                raise MvqError("decode_latents: nb_valid must be a uint8 or bool tensor [B, T_lat]")
            if tuple(nb_valid.shape) != (B, Tlat):
                raise MvqError(f"decode_latents: nb_valid {tuple(nb_valid.shape)} does not match idx's [B={B}, T_lat={Tlat}]")
        if not tactile_only:                 # the audio side must describe the same items as idx (checked before any launch)
            if qa is None:
                if audio_codes is None:
                    raise MvqError("decode_latents: audio_codes (or qa) is required unless tactile_only")
                audio_codes = torch.as_tensor(audio_codes)
                if audio_codes.dim() != 3 or audio_codes.shape[0] != B:
                    raise MvqError(f"decode_latents: audio codes {tuple(audio_codes.shape)} do not match idx's batch B={B}")
            elif qa.dim() != 3 or qa.shape[0] != B or qa.shape[1] != C:
                raise MvqError(f"decode_latents: qa {tuple(qa.shape)} does not match B={B}, C={C}")
            Ta = (audio_codes if qa is None else qa).shape[2]
            if conceal == "plc" and not 0 < Ta <= ops.ATTN_SEQ_MAX_T:
                raise MvqError(f"decode_latents: conceal='plc' needs 1..{ops.ATTN_SEQ_MAX_T} audio tokens, got {Ta}")
        if audio_conceal not in ("zero", "mask", "hold"):
            raise MvqError(f"decode_latents: audio_conceal must be 'zero', 'mask' or 'hold', not {audio_conceal!r}")
        if audio_conceal != "zero" and (tactile_only or qa is not None):
            raise MvqError(f"decode_latents: audio_conceal={audio_conceal!r} conceals the tokens of audio_codes; it goes with neither "
                           "qa nor tactile_only")
        if qa_prev is not None or qa_last_out is not None:
            if audio_conceal != "hold":
                raise MvqError("decode_latents: qa_prev / qa_last_out carry the held audio token; they belong to audio_conceal='hold'")
            if na_valid is None:
                raise MvqError("decode_latents: qa_prev / qa_last_out need na_valid (without it nothing is held)")
            for t, name in ((qa_prev, "qa_prev"), (qa_last_out, "qa_last_out")):
                if t is not None and not (isinstance(t, torch.Tensor) and t.device == dev and t.dtype == torch.float32 and t.dim() == 2
                                          and (qa_slots is not None or t.shape[0] == B) and t.shape[1] == C and t.is_contiguous()):
                    raise MvqError(f"decode_latents: {name} must be a contiguous fp32 tensor [B={B}, C={C}] on {dev}"
                                   + (" (with qa_slots: the pool's [S, C])" if qa_slots is not None else ""))
        if qa_slots is not None or qa_slots_dev is not None:
            if qa_slots is None or qa_prev is None or qa_last_out is None or qa_prev.data_ptr() != qa_last_out.data_ptr():
                raise MvqError("decode_latents: qa_slots address the rows of ONE pool buffer handed in as qa_prev and qa_last_out both")
        if na_valid is None:
            audio_conceal = "zero"                                            # every audio token arrived: nothing to conceal
        if na_valid is not None:
            if tactile_only or qa is not None:
                raise MvqError("decode_latents: na_valid counts the stages of audio_codes; it goes with neither qa nor tactile_only")
            if not isinstance(na_valid, torch.Tensor) or na_valid.dtype not in (torch.uint8, torch.bool):
                raise MvqError("decode_latents: na_valid must be a uint8 or bool tensor [B, Ta]")
            if tuple(na_valid.shape) != (B, audio_codes.shape[2]):
                raise MvqError(f"decode_latents: na_valid {tuple(na_valid.shape)} does not match the codes' [B={B}, Ta={audio_codes.shape[2]}]")
        if B == 0 or Tlat == 0:
            z0 = torch.zeros(B, C, Tlat, device=dev)
            return (z0, torch.zeros(B, C, Ta, device=dev)) if return_qa else z0
        if na_valid is not None:
            na_valid = na_valid.to(dev).contiguous()
            if na_valid.dtype == torch.bool:                                  # all or none: 255 caps at the stages there are
                na_valid = na_valid.view(torch.uint8) * 255
        if nb_valid is not None:
            nb_valid = nb_valid.to(dev).contiguous()
            if nb_valid.dtype == torch.bool:                                  # all or none: 255 caps at the books there are
                nb_valid = nb_valid.view(torch.uint8) * 255
        if tactile_only:                                                      # z_pred absent, as in the transmitter
            z_run = self._pu(self.vq.from_indices(idx, books_use, nb_valid=nb_valid))
            return z_run if conceal == "predict" else ops.plc_mask_fill(z_run, None, nb_valid == 0)[0]
        if qa is None:
            qa = self.A_QUANT.from_codes(audio_codes.to(dev), nq_valid=na_valid)[0]
        qa = ops._dev(qa.to(dev), "qa")                                       # fp32, contiguous
        if qa.shape[0] != B or qa.shape[1] != C:
            raise MvqError(f"decode_latents: qa {tuple(qa.shape)} does not match B={B}, C={C}")
        key_mask = None
        if audio_conceal == "hold":
            carry = None                                                      # read, then moved on in place, by hold_fill_
            if qa_slots is not None:
                ops.hold_fill_(qa, na_valid, qa_last_out, slots=qa_slots, slots_dev=qa_slots_dev)
            elif qa_last_out is not None:
                carry = qa_last_out
                if qa_prev is None:
                    carry.zero_()
                elif qa_prev.data_ptr() != carry.data_ptr():
                    carry.copy_(qa_prev)
            elif qa_prev is not None:
                carry = qa_prev.clone()                                       # qa_prev itself stays as it was handed in
            if qa_slots is None:
                ops.hold_fill_(qa, na_valid, carry)
        elif audio_conceal == "mask":
            key_mask = na_valid                                               # nonzero = at least one stage arrived: a key
        z_run = self._rx_two_pass(qa, idx, books_use, nb_valid, z_prev, key_mask=key_mask)
        if z_last_out is not None:                                            # before the post-pass: what the recursion reads
            ops.copy_strided_(z_last_out, 0, (C, 1), z_run, Tlat - 1, (C * Tlat, Tlat), B, C, 1)
        if conceal == "predict":
            return (z_run, qa) if return_qa else z_run
        lost = nb_valid == 0
        if conceal == "zero":
            z_run = ops.plc_mask_fill(z_run, None, lost)[0]                   # z_run * ~lost
            return (z_run, qa) if return_qa else z_run
        zt_in, _ = ops.plc_mask_fill(z_run, None, lost)                       # what AllPredPLC's predictor is fed
        if key_mask is not None:                                              # the PLC predictor sees what the AR predictor saw
            z_plc = plc.predict(zt_in, qa, key_mask=key_mask)
        else:
            z_plc = plc.predict(zt_in, qa)
        z_run = ops.plc_mask_fill(z_run, z_plc, lost, want_zt_in=False)[1]
        return (z_run, qa) if return_qa else z_run

    def _rx_two_pass(self, qa, idx, books_use, nb_valid=None, z_prev=None, key_mask=None):
        """Layout: every [.., B*Tlat] tensor of the plan is token-folded and PADDED per chunk -- column (b*NC + c)*16 + i holds
        token c*16 + i of item b (NC chunks, the tail chunk's columns past its end are filler) -- so "chunk" is a batch index of
        stride 16 and every chunk with 16 queries and 16 keys is ONE attention call (chunk as batch).  The tail chunk and chunks
        whose audio is shorter (ka < 16, ka = 0: whole-file mode) get calls of their own, which overwrite the big call's
        results for those chunks.  Per-token kernels (LayerNorm, GEMMs) give the same bits whatever the batching.
          pass 1: every token with a zero query input (q = LN(PE[i])), z_run = proj_up(qD) + z_pred;
          pass 2: one query per chunk, input z_run[s-1], attending to its own chunk's keys; the result replaces position 0.
        Chunk 0 takes part in pass 2 with a zero input, recomputing its position 0 exactly as pass 1 did -- or, when this call
        continues a sequence, with ``z_prev`` [B, C], the last token of the piece before (pass 2 then runs for one chunk too).
        ``key_mask`` (uint8 [B, Ta_in], nonzero = the audio token arrived): folded once into the padded key layout ([N] uint8,
        group stride 16, filler 0), so the chunk-as-batch call and the odd-chunk calls of both passes read ONE buffer through the
        masked attention kernel; nothing is read on the host."""
        pr, L = self.predict, self.predict._lin
        B, C, Ta_in = qa.shape
        Tlat = idx.shape[2]
        if idx.shape[1] != B or qa.dtype != torch.float32 or not qa.is_contiguous():
            raise MvqError("_rx_two_pass: qa must be contiguous fp32 with idx's batch")   # every buffer below is sized from B
        CH = AR_CHUNK_TOK
        NC = (Tlat + CH - 1) // CH
        P, G = NC * CH, B * NC
        N = B * P
        dev = qa.device
        Ta = min(Ta_in, Tlat)
        ka = [min(Ta, min(Tlat, s + CH)) - min(Ta, s) for s in range(0, Tlat, CH)]
        nt = [min(Tlat, s + CH) - s for s in range(0, Tlat, CH)]
        odd = [c for c in range(NC) if nt[c] != CH or ka[c] != CH]
        # K, V of every chunk (PosEnc restarts per chunk: column i of a group takes pe[i])
        qa_p = (torch.zeros if Ta < P else torch.empty)(1, C, N, device=dev)
        ops.copy_strided_(qa_p, 0, (P, N), qa, 0, (C * Ta_in, Ta_in), B, C, Ta)
        kv = ops.layernorm_c(qa_p, pr.ln_kv.weight.detach(), pr.ln_kv.bias.detach(), pe=pr.pos.pe, eps=pr.ln_kv.eps, folded_batch=G)
        K, V = L["k"](kv), L["v"](kv)
        km = None
        if key_mask is not None:
            if tuple(key_mask.shape) != (B, Ta_in) or key_mask.dtype != torch.uint8 or key_mask.device != dev:
                raise MvqError(f"_rx_two_pass: key_mask must be uint8 [B={B}, Ta={Ta_in}] on {dev}")
            if Ta_in == P:
                km = key_mask.contiguous().view(-1)                           # already the padded layout
            else:
                km = torch.zeros(B, P, device=dev, dtype=torch.uint8)
                km[:, :Ta].copy_(key_mask[:, :Ta])                            # nonzero = present; filler and missing audio: 0
                km = km.view(-1)
        # qD of every token in one dequantisation
        qD_p = torch.empty(1, CODE_DIM, N, device=dev)
        self.vq.from_indices(idx, books_use, out=qD_p, out_strides=(P, N), nb_valid=nb_valid)   # loss changes qD alone

        def attend(Q, tq, q_strides, q_col_of):
            ctx = torch.empty_like(Q)
            if len(odd) < NC:
                ops.attention_into_(ctx, Q, K, V, pr.h, G, tq, CH, q_strides, (CH, N), kmask=km)
            for c in odd:
                ops.attention_into_(ctx, Q, K, V, pr.h, B, min(tq, nt[c]), ka[c], (q_strides[0] * NC, q_strides[1]), (P, N),
                                    q_col=q_col_of(c), k_col=c * CH, kmask=km)
            return ctx

        # pass 1
        zero = torch.zeros(1, C, N, device=dev)
        z_pred = pr.run(zero, None, folded_batch=G, attend=lambda Q: attend(Q, CH, (CH, N), lambda c: c * CH))
        z_run_p = self._pu(qD_p, residual=z_pred)
        # pass 2: column b*NC + c <- z_run[b, :, c*16 - 1] (zero for c = 0)
        if NC > 1 or z_prev is not None:
            x2 = torch.empty(1, C, G, device=dev)
            ops.copy_strided_(x2, 1, (1, G), z_run_p, CH - 1, (CH, N), G - 1, C, 1)
            if z_prev is None:
                ops.copy_strided_(x2, 0, (NC, G), zero, 0, (0, 0), B, C, 1)
            else:
                ops.copy_strided_(x2, 0, (NC, G), z_prev, 0, (C, 1), B, C, 1)
            z_pred2 = pr.run(x2, None, folded_batch=G, attend=lambda Q: attend(Q, 1, (1, G), lambda c: c))
            qD2 = torch.empty(1, CODE_DIM, G, device=dev)
            ops.copy_strided_(qD2, 0, (1, G), qD_p, 0, (CH, N), G, CODE_DIM, 1)
            z2 = self._pu(qD2, residual=z_pred2)
            ops.copy_strided_(z_run_p, 0, (CH, N), z2, 0, (1, G), G, C, 1)
        z_run = torch.empty(B, C, Tlat, device=dev)
        ops.copy_strided_(z_run, 0, (C * Tlat, Tlat), z_run_p, 0, (P, N), B, C, Tlat)
        return z_run

    def _ar_latents_train(self, qa, zt):
        """The same loop recorded for autograd: z_hat of chunk c feeds column 0 of chunk c+1's zt_prev WITH gradient
        (the reference writes z_hat into z_run in place and slices it back, Training/...5.py:303-319)."""
        B, C, Tlat = zt.shape
        dev = zt.device
        ln = self.tokennorm.ln
        scale_raw = self._scale_raw()
        books = self.vq.stacked()
        chunks, r_toks, prev = [], [], None
        for s in range(0, Tlat, AR_CHUNK_TOK):
            e = min(Tlat, s + AR_CHUNK_TOK)
            n = e - s
            zt_c = ops.fold_time_slice(zt, s, e)
            if prev is None:
                zt_prev = torch.zeros(1, C, B * n, device=dev, dtype=torch.float32)
            else:
                last = prev.reshape(C, B, -1)[:, :, -1:]                                 # z_run[..., s-1], with graph
                zt_prev = torch.cat([last, torch.zeros(C, B, n - 1, device=dev)], dim=2).reshape(1, C, B * n)
            ka = min(qa.shape[-1], e) - min(qa.shape[-1], s)
            qa_c = ops.fold_time_slice(qa, s, s + ka) if ka > 0 else torch.zeros(1, C, 0, device=dev)
            z_pred = self.predict.run_train(zt_prev, qa_c, B)
            r = ops.sub(zt_c, z_pred.detach())
            u = train.LayerNormC.apply(r, ln.weight, ln.bias, None, ln.eps, B)
            rN = train.ScaleTanh.apply(u, self.scale, scale_raw)
            rD = train.Linear.apply(rN, self.proj_down.weight, self.proj_down.bias, None, self._pd)
            qD = train.RvqSte.apply(rD, books, None)
            z_hat = train.Linear.apply(qD, self.proj_up.weight, self.proj_up.bias, z_pred, self._pu)
            chunks.append(z_hat.reshape(C, B, n))
            r_toks.append(rD.detach().reshape(CODE_DIM, B, n))
            prev = z_hat
        z_run = torch.cat(chunks, dim=2).permute(1, 0, 2).contiguous()
        r_tokens = torch.cat(r_toks, dim=2).permute(1, 0, 2).contiguous()
        return z_run, r_tokens


class ProposedEval(_ProposedBase):
    """Evaluation/dac_vcpwq_proposed6_latency.py:437-487."""

    @torch.no_grad()
    def encode_latents(self, a_1T, t_1T, books_use=None):
        qa, zt = self._encode_branches(a_1T, t_1T)
        return self._ar_latents(qa, zt, books_use)[0]

    @torch.no_grad()
    def forward_eval(self, a_1T, t_1T, books_use=None):
        return self.T_DEC(self.encode_latents(a_1T, t_1T, books_use=books_use))

    @torch.no_grad()
    def encode_latents_tactile_only(self, t_1T, books_use=None):
        """BASELINE.json configs[1]: the tactile-side chain with z_pred == 0:
        T_ENC -> tanh(TokenNorm)*scale -> proj_down -> RVQ -> proj_up."""
        zt = self.T_ENC(t_1T)
        z_run, _ = self._ar_latents(None, zt, books_use, tactile_only=True)
        return z_run

    @torch.no_grad()
    def forward_eval_tactile_only(self, t_1T, books_use=None):
        return self.T_DEC(self.encode_latents_tactile_only(t_1T, books_use))


    # ---------------------------------------------------------------------------------------------------------- receiver
    @torch.no_grad()
    def decode(self, audio_codes, idx, books_use=None, nb_valid=None, conceal="predict", plc=None, na_valid=None, audio_conceal="zero"):
        """Receiver: T_DEC(decode_latents(audio_codes, idx)) -- the waveform from the transmitted codes alone.  ``nb_valid`` /
        ``conceal`` / ``plc`` / ``na_valid`` / ``audio_conceal``: the lossy-channel arguments of decode_latents."""
        return self.T_DEC(self.decode_latents(audio_codes, idx, books_use=books_use, nb_valid=nb_valid, conceal=conceal, plc=plc,
                                              na_valid=na_valid, audio_conceal=audio_conceal))

    # ------------------------------------------------------------------------------------- receiver audio output (section 27)
    @property
    def audio_decoder(self):
        """The audio DAC's decoder (set_audio_decoder), or None: what turns the received audio codes into a waveform."""
        return self.__dict__.get("_audio_decoder")

    def __setattr__(self, name, value):                    # nn.Module would register a Module assigned here, past the property
        if name == "audio_decoder":
            raise AttributeError("ProposedEval.audio_decoder is read-only: set_audio_decoder(dec) attaches it outside the state dict")
        super().__setattr__(name, value)

    def set_audio_decoder(self, dec):
        """Attach the audio DAC's decoder for the receiver's audio output (decode_av, decompress_packets_av(audio_out=True),
        stream_receiver(audio_out=True)).  ``dec``: a dac.Decoder with T_DEC's geometry (ValueError otherwise); it is moved to the
        model's device and frozen here.  It is NOT a submodule: checkpoints hold no key of it, so state_dict() and
        load_state_dict(strict=True) are what they are without it, and .to() / .eval() on the model do not reach it -- its weights
        come from the audio DAC's own checkpoint, loaded by the caller.  None detaches it."""
        from .dac import Decoder
        if dec is not None:
            if not isinstance(dec, Decoder):
                raise ValueError(f"set_audio_decoder: a dac.Decoder is required, not {type(dec).__name__}")
            if tuple(dec._desc) != tuple(self.T_DEC._desc):
                raise ValueError(f"set_audio_decoder: decoder geometry {tuple(dec._desc)} is not T_DEC's {tuple(self.T_DEC._desc)} "
                                 "(input channels, width, rates, output channels, output_padding)")
            dec = dec.to(self.proj_up.weight.device).eval().requires_grad_(False)
        self.__dict__["_audio_decoder"] = dec              # past nn.Module.__setattr__: not registered, not in the state dict
        return self

    def _audio_out_args(self, who, audio_out, audio_fade):
        """The refusals every audio_out entry point shares, before any launch."""
        from .packets import AudioFade
        from .stream import _f32_only
        if audio_fade is not None and not audio_out:
            raise ValueError(f"{who}: audio_fade shapes the audio output; it goes with audio_out=True")
        if not audio_out:
            return
        if self.audio_decoder is None:
            raise ValueError(f"{who}: audio_out needs the audio decoder (set_audio_decoder, or build_proposed(audio_decoder=True))")
        if audio_fade is not None and not isinstance(audio_fade, AudioFade):
            raise ValueError(f"{who}: audio_fade must be a packets.AudioFade or None, not {audio_fade!r}")
        _f32_only(f"{who}(audio_out=True)")

    @torch.no_grad()
    def decode_av(self, audio_codes, idx, books_use=None, nb_valid=None, conceal="predict", plc=None, na_valid=None, audio_conceal="zero",
                  audio_fade=None, audio_out_rate=24000):
        """Receiver, both modalities -> (y_tactile, y_audio): decode(...) and y_audio = fade(audio_decoder(qa)) [B, 1, 320*Ta - 8]
        with qa the audio latent as the predictor saw it (decode_latents(return_qa=True)).  ``audio_fade`` (packets.AudioFade): the
        waveform of tokens with na_valid == 0 fades out and back in (ops.audio_fade_, one launch); None, or na_valid None, skips it.
        ``audio_out_rate`` (the rates stream.native_out_plan admits): y_audio is then
        Resample(24000, audio_out_rate) of that waveform, the definition the streaming sessions' audio output equals."""
        from .stream import native_out_plan
        self._audio_out_args("decode_av", True, audio_fade)
        native_out_plan("decode_av", audio_out_rate)
        z, qa = self.decode_latents(audio_codes, idx, books_use=books_use, nb_valid=nb_valid, conceal=conceal, plc=plc, na_valid=na_valid,
                                    audio_conceal=audio_conceal, return_qa=True)
        y_audio = self.audio_decoder(qa)
        if audio_fade is not None and na_valid is not None and y_audio.shape[-1] > 0:
            valid = na_valid.to(qa.device).contiguous()
            valid = valid.view(torch.uint8) if valid.dtype == torch.bool else valid
            y_audio = ops.audio_fade_(y_audio.contiguous(), valid, ops.audio_fade_state(qa.shape[0], qa.device), audio_fade, 0)
        if int(audio_out_rate) != EVAL_SR:
            from .resample import resample_to
            y_audio = resample_to(y_audio, EVAL_SR, int(audio_out_rate))
        return self.T_DEC(z), y_audio

    @torch.no_grad()
    def decode_latents_tactile_only(self, idx, books_use=None, nb_valid=None, conceal="predict"):
        return self.decode_latents(None, idx, books_use=books_use, tactile_only=True, nb_valid=nb_valid, conceal=conceal)

    @torch.no_grad()
    def decode_tactile_only(self, idx, books_use=None, nb_valid=None, conceal="predict"):
        return self.T_DEC(self.decode_latents_tactile_only(idx, books_use, nb_valid, conceal))

    @torch.no_grad()
    def compress(self, a_1T, t_1T, books_use=None):
        """-> (tactile_payloads, audio_payloads): one bitstream.pack_indices payload per item, the RVQ indices [nb, Tlat] at
        K = n_embed and the 32 audio code rows [32, Ta] at K = the DAC codebook size."""
        from . import bitstream
        _, codes, idx = self.encode_latents_with_indices(a_1T, t_1T, books_use=books_use)
        idx, codes = idx.cpu().numpy(), codes.cpu().numpy()
        k_audio = self.A_QUANT.codebook_size
        return ([bitstream.pack_indices(idx[:, b], self.vq.n_embed) for b in range(idx.shape[1])],
                [bitstream.pack_indices(codes[b], k_audio) for b in range(codes.shape[0])])

    @torch.no_grad()
    def decompress(self, tactile_payloads, audio_payloads, books_use=None):
        """The waveform [B,1,T] from compress()'s payloads (items of one length): unpack, then decode()."""
        from . import bitstream
        if len(tactile_payloads) != len(audio_payloads):
            raise MvqError("decompress: one tactile and one audio payload per item")
        idx = [self._payload(bitstream, p, self.vq.n_embed, "tactile") for p in tactile_payloads]
        codes = [self._payload(bitstream, p, self.A_QUANT.codebook_size, "audio") for p in audio_payloads]
        dev = self.proj_up.weight.device
        idx_t = torch.from_numpy(np.stack(idx, axis=1)).to(dev)
        codes_t = torch.from_numpy(np.stack(codes, axis=0)).to(dev)
        return self.decode(codes_t, idx_t, books_use=books_use)

    @torch.no_grad()
    def compress_packets(self, a_1T, t_1T, books_use=None, packet_tok=None, rate=None, fec=None):
        """-> (infos, tactile_packets, audio_payloads) for a lossy channel: per item the session parameters
        packets.StreamInfo(K, nb, T_lat, packet_tok) (sent reliably out of band), the list of framed packets (``bytes``, packets.py)
        of its RVQ indices, and the audio codes as a v1 payload (the audio stream is assumed delivered, as the reference's PLC
        model does).  The packet bodies of the batch are packed on the device and come back in one device->host copy.

        ``rate`` (packets.Rate): the sender chooses each packet's book count on the device, closed loop
        (encode_latents_with_indices); the counts ride back behind the bodies in the same copy and every packet is cut to its
        count (packets.frame).  StreamInfo.nb stays the books in use; decompress_packets needs no change and returns
        T_DEC(the sender's z_run) exactly.

        ``fec`` (packets.Fec; None = today's path and return value): one XOR parity packet per group of ``fec.group`` packets over
        their first ``fec.books`` books (under ``rate``: min(fec.books, the packet's own count)).  The parity rows are computed on the
        device from the packed bodies (ops.fec_parity), ride back behind the bodies and counts in the same single device-to-host
        copy and are framed by packets.frame_fec -> (infos, tactile_packets, audio_payloads, fec_packets), one list of parity
        packets per item; the data packets are byte for byte those of the call without ``fec``.  The closed loop: a recovered packet
        has c_q <= nb_sent[q] books, so the receiver's AR history departs from the sender's exactly as after a relay's ``thin``
        to c_q books, and less than after a loss; with fec.books >= the books in use and at most one deficient packet per group
        (all parity delivered) the receiver's result equals the lossless one bit for bit.  With ``fec.parity = r > 1`` (Reed-Solomon
        over GF(2^8)) every group gets r parity packets, group-major in the item's list -- index 0 the XOR packet unchanged, the
        others with magic ``MR`` -- and "one deficient packet" above reads "at most as many as parity packets of the group arrived"."""
        from . import bitstream, packets
        from .stream import _TxBack
        packet_tok = packets.PACKET_TOK if packet_tok is None else int(packet_tok)
        if fec is not None:
            self._fec_resolve(fec, self.vq.n_embed, self._rate_books(books_use), packet_tok)
        nb_sent = None
        if rate is None:
            _, codes, idx = self.encode_latents_with_indices(a_1T, t_1T, books_use=books_use)
        else:
            _, codes, idx, nb_sent = self.encode_latents_with_indices(a_1T, t_1T, books_use=books_use, rate=rate, packet_tok=packet_tok)
        nb, B, T = idx.shape
        info = packets.StreamInfo(self.vq.n_embed, nb, T, packet_tok)
        back = _TxBack(info.K, nb, packet_tok, counts=rate is not None, fec=fec)   # bodies, the counts under ``rate``, the parity rows
        host = back.pack(idx, nb_sent).cpu().numpy()                           # one copy
        codes = codes.cpu().numpy()
        framed = [back.frame_item(host[b], T) for b in range(B)]
        out = ([info] * B, [f[0] for f in framed], [bitstream.pack_indices(codes[b], self.A_QUANT.codebook_size) for b in range(B)])
        return out if fec is None else out + ([f[1] for f in framed],)

    @torch.no_grad()
    def decompress_packets(self, infos, tactile_packets, audio_payloads, books_use=None, conceal="predict", plc=None, fec=None,
                           fec_packets=None):
        """-> (y [B,1,T], lost [B,T_lat] bool) from whatever packets arrived (missing, reordered, duplicated, thinned; items of
        one StreamInfo): packets.gather per item on the host, ONE upload of the bodies and per-packet book counts, the bit
        unpacking on the device, then decode(nb_valid=...).  ``lost``: the tokens no book of which arrived.

        ``fec`` / ``fec_packets`` (packets.Fec and, per item, whatever parity packets arrived; None = today's path): packets.gather_fec
        per item, the parity rows and ``got`` flags appended to the ONE upload, ops.fec_recover (packets.fec_recover, THE rule: a
        group with its parity and exactly one deficient packet gets that packet back at its protected books) in place ahead of
        ops.idx_unpack_packets; everything after is unchanged, and so are the return values -- ``lost`` is what is still lost after
        recovery.  The result equals plain decompress_packets on the list in which every recovered packet is replaced by
        packets.thin(sent_packet, c_q): the receiver's history departs from the sender's as after that thinning, less than after
        the loss; with fec.books >= the books in use and at most one deficient packet per group it equals the lossless result.
        With ``fec.parity = r > 1`` the upload carries r rows per group and ``got`` as a bitmask of the arrived parity indices; a
        group gets back any d <= (arrived parities) deficient packets, still in the one launch."""
        from . import bitstream, packets
        from .stream import _RxFront
        if fec is None and fec_packets is not None:
            raise MvqError("decompress_packets: fec_packets needs fec=, the packets.Fec both ends agreed on")
        if not (len(infos) == len(tactile_packets) == len(audio_payloads)):
            raise MvqError("decompress_packets: one StreamInfo, one packet list and one audio payload per item")
        dev = self.proj_up.weight.device
        B = len(infos)
        if B == 0:
            raise MvqError("decompress_packets: no items")
        info = packets.StreamInfo(*infos[0])
        if any(tuple(i) != tuple(info) for i in infos):
            raise ValueError("decompress_packets: the items of a batch must share one StreamInfo")
        if info.K != self.vq.n_embed:
            raise ValueError(f"decompress_packets: the stream has K = {info.K}, the model's codebook has {self.vq.n_embed}")
        if fec is not None:
            self._fec_resolve(fec, info.K, info.nb, info.packet_tok)
        none = [None] * B
        front = _RxFront(info.K, info.nb, info.packet_tok, fec=fec)           # bodies, then nb_recv (then parity rows, flags): one upload
        lay, host = self._rx_host(front, B, info.T, tactile_packets, none, self._fec_packets(fec, fec_packets, B, "decompress_packets"), none)
        codes = [self._payload(bitstream, p, self.A_QUANT.codebook_size, "audio") for p in audio_payloads]
        idx, nb_valid, _, _ = front.unpack(torch.from_numpy(host).to(dev), lay, B, info.T)
        codes_t = torch.from_numpy(np.stack(codes, axis=0)).to(dev)
        y = self.decode(codes_t, idx, books_use=books_use, nb_valid=nb_valid, conceal=conceal, plc=plc)
        return y, nb_valid == 0

    @torch.no_grad()
    def compress_packets_av(self, a_1T, t_1T, books_use=None, packet_tok=None, rate=None, audio_books=None, audio_rate=None, fec=None,
                            audio_fec=None):
        """compress_packets with the audio codes in layered packets too -> (infos, tactile_packets, audio_infos, audio_packets).
        The audio stream uses the tactile stream's format unchanged: per item StreamInfo(K = A_QUANT.codebook_size,
        nb = audio_books, Ta, packet_tok) and the framed packets of codes[b, :audio_books] (stage-major bodies: dropping the later
        stages of an audio packet is a truncation).  One ``packet_tok`` serves both streams; they are told apart by the list they
        travel in.  The sender runs closed on both streams (encode_latents_with_indices; ``rate`` / ``audio_rate`` None = every
        packet whole).  Both sets of bodies are packed on the device and come back with both sets of counts in ONE device->host
        copy; packets.frame cuts each packet to its count.  decompress_packets_av with nothing lost returns T_DEC(the sender's
        z_run) exactly.

        ``fec`` / ``audio_fec`` (packets.Fec per stream; both None = today's path and return value): compress_packets(fec=) per
        stream -- on the audio stream ``Fec.books`` counts stages -- the parity rows of both computed on the device from the packed
        bodies and the device-side counts, still ONE device->host copy.  With either given the call returns the four elements and
        then (fec_packets, audio_fec_packets), per item one list of parity packets per stream; a stream without a Fec gets empty
        lists.  The closed loop: as compress_packets(fec=) says, on each stream."""
        from . import packets
        from .stream import _TxBack
        audio_rate, na_use, packet_tok = self._audio_rate_resolve(audio_rate, audio_books, packet_tok)
        if fec is not None:
            self._fec_resolve(fec, self.vq.n_embed, self._rate_books(books_use), packet_tok)
        if audio_fec is not None:
            self._fec_resolve(audio_fec, self.A_QUANT.codebook_size, na_use, packet_tok, what="audio_fec")
        _, codes, idx, nb_sent, na_sent = self.encode_latents_with_indices(a_1T, t_1T, books_use=books_use, rate=rate, packet_tok=packet_tok,
                                                                           audio_books=na_use, audio_rate=audio_rate)
        nb, B, T = idx.shape
        info = packets.StreamInfo(self.vq.n_embed, nb, T, packet_tok)
        ainfo = packets.StreamInfo(self.A_QUANT.codebook_size, na_use, codes.shape[2], packet_tok)
        back = _TxBack(info.K, nb, packet_tok, (ainfo.K, na_use), fec=fec, audio_fec=audio_fec)
        host = back.pack(idx, nb_sent, codes, na_sent).cpu().numpy()
        framed = [back.frame_item(host[b], T) for b in range(B)]
        tp, ap, *parity = ([f[i] for f in framed] for i in range(2 if fec is None and audio_fec is None else 4))
        return ([info] * B, tp, [ainfo] * B, ap, *parity)

    @torch.no_grad()
    def decompress_packets_av(self, infos, tactile_packets, audio_infos, audio_packets, books_use=None, conceal="predict", plc=None,
                              fec=None, fec_packets=None, audio_fec=None, audio_fec_packets=None, audio_conceal="zero", audio_out=False,
                              audio_fade=None, audio_out_rate=24000):
        """-> (y [B,1,T], lost [B,T_lat] bool, audio_lost [B,Ta] bool) from whatever packets of BOTH streams arrived (missing,
        reordered, duplicated, thinned; items of one StreamInfo per stream): packets.gather per item and stream on the host, ONE
        upload of both streams' bodies and per-packet counts, the bit unpacking of both on the device (the audio indices are
        transposed to codes[B, nq, Ta] there), then decode(nb_valid=, na_valid=).  ``audio_lost``: the audio tokens no stage of
        which arrived; they are +0 to the predictor, or concealed as ``audio_conceal`` says ("zero" / "mask" / "hold":
        decode_latents; what FEC recovered is not lost and is not concealed).

        ``fec`` / ``fec_packets`` / ``audio_fec`` / ``audio_fec_packets``: decompress_packets(fec=) per stream -- packets.gather_fec per
        item and stream, the parity rows and ``got`` flags of both behind the existing arrays in the ONE upload, ops.fec_recover on
        each stream ahead of its ops.idx_unpack_packets.  The return values do not change; ``lost`` / ``audio_lost`` are what is still
        lost after recovery.  The closed loop: as decompress_packets(fec=) says, on each stream.

        ``audio_out=True`` (needs set_audio_decoder): -> (y, lost, audio_lost, y_audio), the first three exactly as
        without it and y_audio [B, 1, 320*Ta - 8] the audio waveform, decode_av's: the audio decoder on the audio latent the predictor
        saw, then ``audio_fade`` (packets.AudioFade or None) over the tokens that are still lost after recovery.  ``audio_out_rate``
        (decode_av's; needs audio_out=True): y_audio resampled from 24 kHz to that rate."""
        from . import packets
        from .stream import _RxFront, native_out_plan
        self._audio_out_args("decompress_packets_av", audio_out, audio_fade)
        native_out_plan("decompress_packets_av", audio_out_rate, audio_out)
        if audio_conceal not in ("zero", "mask", "hold"):
            raise MvqError(f"decompress_packets_av: audio_conceal must be 'zero', 'mask' or 'hold', not {audio_conceal!r}")
        if (fec is None and fec_packets is not None) or (audio_fec is None and audio_fec_packets is not None):
            raise MvqError("decompress_packets_av: fec_packets / audio_fec_packets need fec= / audio_fec=, the packets.Fec both ends agreed on")
        if not (len(infos) == len(tactile_packets) == len(audio_infos) == len(audio_packets)):
            raise MvqError("decompress_packets_av: one StreamInfo and one packet list per item and stream")
        dev = self.proj_up.weight.device
        B = len(infos)
        if B == 0:
            raise MvqError("decompress_packets_av: no items")
        info, ainfo = packets.StreamInfo(*infos[0]), packets.StreamInfo(*audio_infos[0])
        if any(tuple(i) != tuple(info) for i in infos) or any(tuple(i) != tuple(ainfo) for i in audio_infos):
            raise ValueError("decompress_packets_av: the items of a batch must share one StreamInfo per stream")
        if info.K != self.vq.n_embed:
            raise ValueError(f"decompress_packets_av: the tactile stream has K = {info.K}, the model's codebook has {self.vq.n_embed}")
        if ainfo.K != self.A_QUANT.codebook_size or not 1 <= ainfo.nb <= self.A_QUANT.n_codebooks:
            raise ValueError(f"decompress_packets_av: the audio stream has K = {ainfo.K}, nb = {ainfo.nb}; the model's audio quantiser "
                             f"has K = {self.A_QUANT.codebook_size} and {self.A_QUANT.n_codebooks} stages")
        if ainfo.packet_tok != info.packet_tok:
            raise ValueError(f"decompress_packets_av: one packet_tok serves both streams, got {info.packet_tok} and {ainfo.packet_tok}")
        if ainfo.T != info.T:
            raise ValueError(f"decompress_packets_av: the audio stream has T = {ainfo.T} tokens, the tactile stream {info.T}; the two "
                             "modalities advance together")
        parity = []
        for f, fp, inf, what in ((fec, fec_packets, info, "fec"), (audio_fec, audio_fec_packets, ainfo, "audio_fec")):
            if f is not None:
                self._fec_resolve(f, inf.K, inf.nb, inf.packet_tok, what=what)
            parity.append(self._fec_packets(f, fp, B, "decompress_packets_av", what))
        front = _RxFront(info.K, info.nb, info.packet_tok, (ainfo.K, ainfo.nb), fec, audio_fec)
        lay, host = self._rx_host(front, B, info.T, tactile_packets, audio_packets, *parity)   # both streams' arrays: one upload
        idx, nb_valid, codes, na_valid = front.unpack(torch.from_numpy(host).to(dev), lay, B, info.T)
        if audio_out:
            y, y_audio = self.decode_av(codes, idx, books_use=books_use, nb_valid=nb_valid, conceal=conceal, plc=plc, na_valid=na_valid,
                                        audio_conceal=audio_conceal, audio_fade=audio_fade, audio_out_rate=audio_out_rate)
            return y, nb_valid == 0, na_valid == 0, y_audio
        y = self.decode(codes, idx, books_use=books_use, nb_valid=nb_valid, conceal=conceal, plc=plc, na_valid=na_valid,
                        audio_conceal=audio_conceal)
        return y, nb_valid == 0, na_valid == 0

    def stream_receiver(self, K, nb, packet_tok=2, batch=1, books_use=None, conceal="predict", out_rate=24000, graph=False, audio=None,
                        fec=None, audio_fec=None, audio_conceal="zero", decoder="window", audio_out=False, audio_fade=None,
                        audio_out_rate=24000):
        """A streaming session on this model (stream.StreamReceiver): ``push`` one 16-token chunk of packets and audio codes at a
        time, ``finish`` to flush; the concatenated output equals decompress_packets on the same packets bit for bit.
        ``decoder="stateful"``: the same tensors from the stateful decoder (per-stage history instead of the 36-token window).
        ``audio_out=True`` (``audio_fade``: packets.AudioFade or None): push / finish return (y_tactile, y_audio), the audio waveform
        chunk by chunk, equal to decompress_packets_av(audio_out=True)'s.  ``audio_out_rate`` (44100, 48000, ...: stream.native_out_plan):
        y_audio at the playback rate, equal to decompress_packets_av(audio_out=True, audio_out_rate=)'s."""
        from .stream import StreamReceiver
        return StreamReceiver(self, K, nb, packet_tok=packet_tok, batch=batch, books_use=books_use, conceal=conceal,
                              out_rate=out_rate, graph=graph, audio=audio, fec=fec, audio_fec=audio_fec, audio_conceal=audio_conceal,
                              decoder=decoder, audio_out=audio_out, audio_fade=audio_fade, audio_out_rate=audio_out_rate)

    def stream_receiver_pool(self, K, nb, packet_tok=2, slots=64, books_use=None, conceal="predict", out_rate=24000, audio_conceal=None,
                             decoder="window"):
        """A pool of up to ``slots`` independent receiver sessions on this model (stream.StreamReceiverPool): ``open`` a
        session, ``step`` once per tick with the chunks that are ready (and the sessions that end); each session gets what a
        stream_receiver(batch=1) of its own would return, and the sessions of a tick share batched launches."""
        from .stream import StreamReceiverPool
        return StreamReceiverPool(self, K, nb, packet_tok=packet_tok, slots=slots, books_use=books_use, conceal=conceal,
                                  out_rate=out_rate, audio_conceal=audio_conceal,    # the pool takes no audio= and refuses an audio_conceal
                                  decoder=decoder)

    def stream_sender(self, packet_tok=2, batch=1, books_use=None, graph=False, rate=None, audio="codes", audio_books=None, audio_rate=None,
                      fec=None, audio_fec=None, encoder="window"):
        """A streaming sender session on this model (stream.StreamSender): ``push`` samples of both modalities as they come,
        get back the packets and audio codes of each 16-token chunk they complete, ``finish`` to flush; the concatenated output
        equals compress_packets on the whole item byte for byte (with ``rate``, a packets.Rate: compress_packets(rate=)).
        ``encoder="stateful"``: the same return values from the stateful encoders (per-stage history instead of the 32-token window)."""
        from .stream import StreamSender
        return StreamSender(self, packet_tok=packet_tok, batch=batch, books_use=books_use, graph=graph, rate=rate, audio=audio,
                            audio_books=audio_books, audio_rate=audio_rate, fec=fec, audio_fec=audio_fec, encoder=encoder)

    def stream_sender_native(self, in_rates=(44100, 3000), **sender_options):
        """stream_sender fed at the sensors' own rates (stream.StreamSenderNative): ``in_rates`` = (audio Hz, tactile Hz),
        ``sender_options`` what stream_sender takes.  ``push`` takes whole tokens of native samples (588 and 40 per token at the
        default rates), ``finish`` the rest; the concatenated output equals compress_packets on the whole item resampled to 24 kHz
        and crop_matched, byte for byte.  Adds one token-time (13.3 ms) of algorithmic latency."""
        from .stream import StreamSenderNative
        return StreamSenderNative(self, in_rates=in_rates, **sender_options)

    def stream_sender_pool(self, packet_tok=2, slots=64, books_use=None, encoder="window"):
        """A pool of up to ``slots`` independent sender sessions on this model (stream.StreamSenderPool): ``open`` a session,
        ``step`` once per tick with the samples that arrived (1..16 tokens per session, and the sessions that end); each
        session gets what a stream_sender(batch=1) of its own would return, and the sessions of a tick share batched encodes."""
        from .stream import StreamSenderPool
        return StreamSenderPool(self, packet_tok=packet_tok, slots=slots, books_use=books_use, encoder=encoder)

    def stream_sender_pool_av(self, packet_tok=2, slots=64, books_use=None, rate=None, audio="packets", audio_books=None, audio_rate=None,
                              fec=None, audio_fec=None, encoder="window"):
        """stream_sender_pool for the whole link (stream.StreamSenderPoolAV): ``rate``, ``audio`` / ``audio_books`` / ``audio_rate``,
        ``fec`` / ``audio_fec`` and ``encoder`` mean what they mean on stream_sender, and each session gets what a
        stream_sender(batch=1) with the same options would return.  ``audio="codes"``: a tactile-only stream with rate= / fec=."""
        from .stream import StreamSenderPoolAV
        return StreamSenderPoolAV(self, packet_tok=packet_tok, slots=slots, books_use=books_use, rate=rate, audio=audio,
                                  audio_books=audio_books, audio_rate=audio_rate, fec=fec, audio_fec=audio_fec, encoder=encoder)

    def stream_receiver_pool_av(self, K, nb, packet_tok=2, slots=64, books_use=None, conceal="predict", out_rate=24000, audio=None,
                                fec=None, audio_fec=None, audio_conceal="zero", decoder="window"):
        """stream_receiver_pool for the whole link (stream.StreamReceiverPoolAV): ``audio=(K_a, na)``, ``fec`` / ``audio_fec``,
        ``audio_conceal`` and ``decoder`` mean what they mean on stream_receiver, and each session gets what a
        stream_receiver(batch=1) with the same options would return.  ``audio=None``: the audio codes arrive as codes.
        The audio output (``audio_out`` / ``audio_fade`` / ``audio_out_rate``, as on stream_receiver) is the class's:
        StreamReceiverPoolAV(net, K, nb, ..., audio_out=True); this factory's signature is pinned as it is."""
        from .stream import StreamReceiverPoolAV
        return StreamReceiverPoolAV(self, K, nb, packet_tok=packet_tok, slots=slots, books_use=books_use, conceal=conceal,
                                    out_rate=out_rate, audio=audio, fec=fec, audio_fec=audio_fec, audio_conceal=audio_conceal,
                                    decoder=decoder)

    @staticmethod
    def _payload(bitstream, payload, k_expected, what):
        idx, k = bitstream.unpack_indices(payload)
        if k != k_expected:
            raise ValueError(f"decompress: {what} payload has K = {k}, the model's codebook has {k_expected}")
        return idx


RVQ_N_BOOKS_MAX = 10  # Evaluation/compare_dacvsproposal_3.5_eval.py:68
RVQ_EMBED = 128       # ...:69


class ProposedWrapper(_ProposedBase):
    """The eval wrapper of Evaluation/compare_dacvsproposal_3.5_eval.py:374-411: constructor
    ``(A_ENC, A_QUANT, T_ENC, T_DEC, c_lat)`` -- the RVQ shape comes from that script's module constants
    ``RVQ_N_BOOKS_MAX = 10`` x ``RVQ_EMBED = 128`` (...:68-69; built at ...:485) -- and ``forward_eval(a, t, books_use)`` with a
    REQUIRED ``books_use`` (swept over 1..3 at ...:504).  Its AR loop writes ``zt_prev[...] = z_run[..., s-1:e-1]`` for
    s > 0 and ``zt_prev[..., 1:] = z_run[..., s:e-1]`` for s == 0 (...:393-396): the entries of z_run read for positions
    1.. have not been written yet, so -- exactly as in the other scripts -- only column 0 of a chunk with s > 0 is non-zero
    and the launch plan is ``_ar_latents`` unchanged."""

    def __init__(self, A_ENC, A_QUANT, T_ENC, T_DEC, c_lat):
        super().__init__(A_ENC, A_QUANT, T_ENC, T_DEC, c_lat, RVQ_N_BOOKS_MAX, RVQ_EMBED)

    @torch.no_grad()
    def forward_eval(self, a_1T, t_1T, books_use: int):
        qa, zt = self._encode_branches(a_1T, t_1T)
        return self.T_DEC(self._ar_latents(qa, zt, int(books_use))[0])


def encoder_out_len(enc, t: int):
    """Latent tokens a dac.Encoder gives for ``t`` samples, from its strides alone (the k = 7 / 3 convs and the ResidualUnits keep
    the length; a block's strided conv has k = 2s, padding ceil(s/2)); None for another kind of module.  Lets the training entry
    points refuse a mask of the wrong length before anything is launched."""
    desc = getattr(enc, "_desc", None)
    if not isinstance(desc, tuple) or len(desc) != 3:
        return None
    t = int(t)
    for s in desc[1]:
        t = (t + 2 * math.ceil(s / 2) - 2 * s) // s + 1
        if t <= 0:
            return 0
    return t


def link_step_refusals(who, net, a_1T, tc_1T, nb_valid, na_valid, audio_conceal, link, tactile=True):
    """The refusals of a training step under a lossy link (AllPredAR / AllPredPLC.forward_step), before any launch."""
    from . import packets
    if audio_conceal not in ("zero", "mask", "hold"):
        raise MvqError(f"{who}: audio_conceal must be 'zero', 'mask' or 'hold', not {audio_conceal!r}")
    if link is not None:
        if not isinstance(link, packets.Link):
            raise MvqError(f"{who}: link must be a packets.Link")
        if nb_valid is not None or na_valid is not None:
            raise MvqError(f"{who}: link draws the masks itself; it goes with neither nb_valid nor na_valid")
    B = a_1T.shape[0]
    for m, name, enc, x in ((nb_valid, "nb_valid", net.T_ENC, tc_1T), (na_valid, "na_valid", net.A_ENC, a_1T)):
        if m is None:
            continue
        if not isinstance(m, torch.Tensor) or m.dtype != torch.uint8:
            raise MvqError(f"{who}: {name} must be a uint8 tensor [B, T]")
        n = encoder_out_len(enc, x.shape[-1])
        if m.dim() != 2 or m.shape[0] != B or (n is not None and m.shape[1] != n):
            raise MvqError(f"{who}: {name} {tuple(m.shape)} does not match [B={B}, T={'?' if n is None else n}]")
        if m.device != x.device:
            raise MvqError(f"{who}: {name} must be on the device of the signals ({x.device}), not {m.device}")
    if audio_conceal != "zero" and na_valid is None and (link is None or link.audio is None):
        raise MvqError(f"{who}: audio_conceal={audio_conceal!r} conceals lost audio tokens; it needs na_valid or a link with an audio channel")


class AllPredAR(_ProposedBase):
    """Training/compare_dacvsproposal_5.py:279-326.  Under ``torch.no_grad()`` (validation, ...:411-414) this is the
    fused inference path; with autograd enabled it records the HIP-backed graph of train.py for ``.backward()``."""

    def _forward_step(self, a_1T, tc_1T):
        Tw = tc_1T.shape[-1]
        with torch.no_grad():                                                  # frozen backbones: no graph
            qa, zt = self._encode_branches(a_1T, tc_1T)
        if torch.is_grad_enabled() and zt.numel() and any(p.requires_grad for p in self.parameters()):
            z_run, r_tokens = self._ar_latents_train(qa, zt)
            y_hat = self.T_DEC(z_run)                                          # _DecoderInputGrad: HIP backward w.r.t. z
        else:
            with torch.no_grad():
                z_run, r_tokens = self._ar_latents(qa, zt, None, want_tokens=True)
                y_hat = self.T_DEC(z_run)
        T = min(y_hat.shape[-1], tc_1T.shape[-1], Tw)
        fz = lambda x: torch.nan_to_num(x, nan=0.0, posinf=0.0, neginf=0.0)   # finite_or_zero (...5.py:99-100)
        return {"y_hat": fz(y_hat[..., :T]), "tgt": fz(tc_1T[..., :T]), "r_tokens": r_tokens}, qa, zt

    def forward_step(self, a_1T, tc_1T, *, nb_valid=None, na_valid=None, audio_conceal="zero", link=None, step=0):
        """With every keyword at its default: the reference's step.  Otherwise the step under a lossy link, closed-loop in the
        RECEIVER's arithmetic: ``nb_valid`` (uint8 [B, T_lat]: the tactile books of each token that arrive, 0 = lost) and
        ``na_valid`` (uint8 [B, Ta]: the audio stages that arrive) as decode_latents takes them, ``audio_conceal`` its three modes,
        or ``link`` (a packets.Link) with ``step``: both masks are drawn on the device (ops.channel_draw, streams 0 and 1).
        Returns the default keys plus "z_run", "idx" [n_books, B, T_lat], "codes", "nb_valid", "na_valid"."""
        if nb_valid is None and na_valid is None and audio_conceal == "zero" and link is None:
            return self._forward_step(a_1T, tc_1T)[0]
        return self._forward_step_link(a_1T, tc_1T, nb_valid, na_valid, audio_conceal, link, step)

    def _forward_step_link(self, a_1T, tc_1T, nb_valid, na_valid, audio_conceal, link, step):
        who = "AllPredAR.forward_step"
        link_step_refusals(who, self, a_1T, tc_1T, nb_valid, na_valid, audio_conceal, link)
        dev = self.proj_up.weight.device
        Tw = tc_1T.shape[-1]
        with torch.no_grad():                                                  # frozen backbones: no graph
            qa, codes, *_ = self.A_QUANT(self.A_ENC(a_1T))
            zt = self.T_ENC(tc_1T)
        B, C, Tlat = zt.shape
        Ta = codes.shape[2]
        nbk = len(self.vq.books)
        if link is not None:
            nb_valid = ops.channel_draw(link.tactile, nbk, Tlat, link.packet_tok, B, stream=0, step=step, device=dev)
            if link.audio is not None:
                na_valid = ops.channel_draw(link.audio, codes.shape[1], Ta, link.packet_tok, B, stream=1, step=step, device=dev)
        if nb_valid is not None and (tuple(nb_valid.shape) != (B, Tlat) or nb_valid.device != zt.device):
            raise MvqError(f"{who}: nb_valid {tuple(nb_valid.shape)} on {nb_valid.device} does not match [B={B}, T_lat={Tlat}] on {zt.device}")
        if na_valid is not None and (tuple(na_valid.shape) != (B, Ta) or na_valid.device != zt.device):
            raise MvqError(f"{who}: na_valid {tuple(na_valid.shape)} on {na_valid.device} does not match the codes' [B={B}, Ta={Ta}] on {zt.device}")
        key_mask = None
        with torch.no_grad():
            if na_valid is not None:
                na_valid = na_valid.contiguous()
                qa = self.A_QUANT.from_codes(codes, nq_valid=na_valid)[0]
                qa = ops._dev(qa, "qa")
                if audio_conceal == "hold":
                    ops.hold_fill_(qa, na_valid)
                elif audio_conceal == "mask":
                    key_mask = na_valid
        nbv = nb_valid.contiguous() if nb_valid is not None else torch.full((B, Tlat), min(nbk, 255), device=zt.device, dtype=torch.uint8)
        z_run, r_tokens, idx = self._ar_latents_link(qa, zt, nbv, key_mask)
        y_hat = self.T_DEC(z_run)
        T = min(y_hat.shape[-1], tc_1T.shape[-1], Tw)
        fz = lambda x: torch.nan_to_num(x, nan=0.0, posinf=0.0, neginf=0.0)
        return {"y_hat": fz(y_hat[..., :T]), "tgt": fz(tc_1T[..., :T]), "r_tokens": r_tokens, "z_run": z_run, "idx": idx,
                "codes": codes, "nb_valid": nb_valid, "na_valid": na_valid}

    def _ar_latents_link(self, qa, zt, nb_valid, key_mask):
        """_ar_latents_train under a lossy link: the quantiser is the layered straight-through one (the receiver's sum of the books
        that arrive), the predictor attends under ``key_mask``, and z_hat -- what the receiver will hold -- feeds the next chunk.
        Under torch.no_grad() the same ops run without recording.  -> (z_run, r_tokens, idx [n_books, B, T_lat])."""
        B, C, Tlat = zt.shape
        dev = zt.device
        ln = self.tokennorm.ln
        scale_raw = self._scale_raw()
        books = self.vq.stacked()
        chunks, r_toks, idxs, prev = [], [], [], None
        for s in range(0, Tlat, AR_CHUNK_TOK):
            e = min(Tlat, s + AR_CHUNK_TOK)
            n = e - s
            zt_c = ops.fold_time_slice(zt, s, e)
            if prev is None:
                zt_prev = torch.zeros(1, C, B * n, device=dev, dtype=torch.float32)
            else:
                last = prev.reshape(C, B, -1)[:, :, -1:]                                 # z_run[..., s-1], with graph
                zt_prev = torch.cat([last, torch.zeros(C, B, n - 1, device=dev)], dim=2).reshape(1, C, B * n)
            ka = min(qa.shape[-1], e) - min(qa.shape[-1], s)
            qa_c = ops.fold_time_slice(qa, s, s + ka) if ka > 0 else torch.zeros(1, C, 0, device=dev)
            km_c = key_mask[:, s:s + ka].contiguous() if (key_mask is not None and ka > 0) else None
            z_pred = self.predict.run_train(zt_prev, qa_c, B, key_mask=km_c)
            r = ops.sub(zt_c, z_pred.detach())
            u = train.LayerNormC.apply(r, ln.weight, ln.bias, None, ln.eps, B)
            rN = train.ScaleTanh.apply(u, self.scale, scale_raw)
            rD = train.Linear.apply(rN, self.proj_down.weight, self.proj_down.bias, None, self._pd)
            qD, idx_c = train.RvqSteLayers.apply(rD, books, nb_valid[:, s:e].contiguous())
            z_hat = train.Linear.apply(qD, self.proj_up.weight, self.proj_up.bias, z_pred, self._pu)
            chunks.append(z_hat.reshape(C, B, n))
            r_toks.append(rD.detach().reshape(CODE_DIM, B, n))
            idxs.append(idx_c.reshape(-1, B, n))
            prev = z_hat
        if not chunks:
            z = torch.zeros(B, C, 0, device=dev)
            return z, torch.zeros(B, CODE_DIM, 0, device=dev), torch.zeros(len(self.vq.books), B, 0, device=dev, dtype=torch.int64)
        z_run = torch.cat(chunks, dim=2).permute(1, 0, 2).contiguous()
        r_tokens = torch.cat(r_toks, dim=2).permute(1, 0, 2).contiguous()
        return z_run, r_tokens, torch.cat(idxs, dim=2).contiguous()


class AllPredAR3(AllPredAR):
    """The ``AllPredAR`` of Training/compare_dacvsproposal_3.py:278-340 (BASELINE.json configs[0]): same model, but the
    constructor takes no sweep arguments (the script's module constants RVQ_N_BOOKS = 10, RVQ_EMBED = 128, ...:61-63) and
    ``forward_step`` additionally returns ``z_teacher`` (= T_ENC(tc), indexed by the script's ``step()``, ...:389-394) and
    ``z_pred`` (one more ``predict()`` call on an all-zero ``zt_prev`` over the first chunk, ...:334-337 -- unused by the
    loss, but in train mode it draws one more dropout mask, so it is issued at the same point of the RNG stream)."""

    def __init__(self, A_ENC, A_QUANT, T_ENC, T_DEC, c_lat, rvq_books: int = 10, rvq_embed: int = 128, decay=EMA_DECAY):
        super().__init__(A_ENC, A_QUANT, T_ENC, T_DEC, c_lat, rvq_books, rvq_embed, decay)

    def forward_step(self, a_1T, tc_1T):
        out, qa, zt = self._forward_step(a_1T, tc_1T)
        Tlat = zt.shape[-1]
        n = min(AR_CHUNK_TOK, Tlat)
        z_pred = None
        if Tlat > 0:
            ka = min(qa.shape[-1], n)
            z_pred = self.predict(torch.zeros_like(zt[..., :n]), qa[..., :ka].contiguous())
        return {"y_hat": out["y_hat"], "tgt": out["tgt"], "z_pred": z_pred, "z_teacher": zt,
                "r_tokens": out["r_tokens"] if Tlat > 0 else None}


def psnr_batch(ref_1T, est_1T, eps=1e-12):
    """PSNR(dB), peak = 1.0 (Evaluation/compare_dacvsproposal_5_eval.py:180-185)."""
    ref = ref_1T.to(torch.float32); est = est_1T.to(torch.float32)
    mse = (ref - est).pow(2).mean(dim=(1, 2)).clamp_min(eps)
    return [float(v) for v in (10.0 * torch.log10(1.0 / mse)).cpu()]


def psnr_global_peak_db(ref, est, peak, eps=1e-12):
    """Evaluation/dac_vcpwq_proposed6_latency.py:204-214."""
    ref = ref.reshape(-1).to(torch.float32); est = est.reshape(-1).to(torch.float32)
    mse = torch.mean((ref - est) ** 2) + eps
    peak = max(float(peak), eps)
    return float(10.0 * torch.log10((peak * peak) / mse).cpu())


def crop_match(a_1T, b_1T):
    """Evaluation/dac_vcpwq_proposed6_latency.py:158-160."""
    T = min(a_1T.shape[-1], b_1T.shape[-1])
    return a_1T[..., :T], b_1T[..., :T]


@torch.no_grad()
def align_by_xcorr(ref_1T, est_1T, max_shift=200):
    """Evaluation/dac_vcpwq_proposed6_latency.py:164-202: align est to ref by the integer shift that maximises the
    cross-correlation.  All 2*max_shift+1 correlations run in one launch; ONE device->host read (the shift)."""
    r = ref_1T.reshape(-1).to(torch.float32); e = est_1T.reshape(-1).to(torch.float32)
    _, best = ops.align_xcorr(r, e, max_shift)
    s = int(best.item())
    if s < 0:
        r_a = r[-s:]; e_a = e[: r_a.numel()]
    elif s > 0:
        r_a = r[:-s]; e_a = e[s: s + r_a.numel()]
    else:
        r_a = r; e_a = e[: r.numel()]
    return r_a.unsqueeze(0), e_a.unsqueeze(0), s


ALIGN_MAX_SHIFT_SAMPLES = 200      # Evaluation/compare_dacvsproposal_5_eval.py:69
EVAL_SR, ORIG_3K = 24000, 3000     # ...:52-53


@torch.no_grad()
def align_pair_24k(ref_24, est_24, max_shift=ALIGN_MAX_SHIFT_SAMPLES):
    """Evaluation/compare_dacvsproposal_5_eval.py:188-210 ([1,1,T] in, [1,1,T'] out)."""
    r_a, e_a, s = align_by_xcorr(ref_24.reshape(1, -1), est_24.reshape(1, -1), max_shift)
    return r_a.unsqueeze(0), e_a.unsqueeze(0), s


_DOWN_3K = {}          # device -> Resample(24 000, 3 000): the filter bank is designed once, not once per call


@torch.no_grad()
def psnr_3k_aligned_batch(ref_24, est_24, max_shift=ALIGN_MAX_SHIFT_SAMPLES):
    """Evaluation/compare_dacvsproposal_5_eval.py:212-223: per item, align at 24 kHz (+-200 samples), resample both to
    3 kHz, PSNR with peak 1.  Three launches for the whole batch and ONE device->host copy (the B PSNR values): the B
    alignments run in one launch pair (grid dimension = item), the slice bounds each shift implies (...:196-207) are computed
    on the device, the 2B ragged slices are resampled in one launch (mvq_resample_ragged_f32), and the squared error is
    reduced per row on the device.  (The reference syncs 401 + 1 times per item.)"""
    from .resample import Resample
    ref = ref_24.reshape(ref_24.shape[0], -1).to(torch.float32).contiguous()
    est = est_24.reshape(est_24.shape[0], -1).to(torch.float32).contiguous()
    B, T = ref.shape
    if B == 0:
        return []
    dev = ref.device
    s = ops.align_xcorr_batch(ref, est, max_shift)                       # int32 [B], stays on the device
    length = (T - s.abs()).to(torch.int32)                               # both aligned slices have T - |s| samples
    zero = torch.zeros_like(s)
    off = torch.cat([torch.maximum(-s, zero), torch.maximum(s, zero)]).to(torch.int32)     # ref starts at -s (s < 0), est at s (s > 0)
    down = _DOWN_3K.get(str(dev))
    if down is None:
        down = _DOWN_3K[str(dev)] = Resample(EVAL_SR, ORIG_3K).to(dev)
    pitch = (down.new * T + down.orig - 1) // down.orig
    y, lout = ops.resample_ragged(torch.cat([ref, est]), down.kernel, off, torch.cat([length, length]), down.orig, down.new,
                                  down.width, pitch)
    n3 = lout[:B].to(torch.float32).clamp_min(1.0)
    mse = ((y[:B] - y[B:]).pow(2).sum(dim=1) / n3).clamp_min(1e-12)    # rows are zero past their length on both sides
    return [float(v) for v in (10.0 * torch.log10(1.0 / mse)).cpu()]
