"""Streaming receiver: the tactile waveform chunk by chunk, bit-equal to the whole-item ``decompress_packets``.

The whole-item receiver waits for every token of an item before the first sample leaves it.  Nothing in the model needs that:

  * latents -- a 16-token chunk depends on the earlier ones through ONE token, z_run[..., s-1], which
    ``decode_latents(z_prev=, z_last_out=)`` carries in a fixed [B, C] device buffer;
  * decoder -- T_DEC is a finite-support conv stack.  Decoding the token window [a, b) reproduces the whole-sequence output bit for
    bit at global sample 320*a + i, except for the first DEC_HALO_SAMPLES[0] and the last DEC_HALO_SAMPLES[1] samples of the
    window; a window edge that is the true sequence edge is exact.  A halo of DEC_HALO_TOK tokens on each side covers both.

Where the constants come from: measured on the CPU oracle (oracle.dac_decoder, synth.dac_state(seed=7) decoder weights, seeded
random latents [2, 1024, T]) by decoding windows of a sequence and comparing with the one-shot decode, sample by sample;
tests/test_stream_cpu.py repeats the part that guards them (the schedule at halo 10 is exact, at halo 9 it is not) and
tests/stream_oracle.py holds the procedure (measure_halo: 3133 at both ends of the window [20, 55) of 75 tokens, counted inside
the window's 320*(b-a) - 8 output samples; 3141 is that extent counted from the nominal edge 320*b, and the count at the start
moves by a sample with the data).  The schedule's margins are 3200 samples at a window start and 3192 at a window end.  The
extents are properties of the architecture (kernel sizes, dilations, strides), not of the weights.  ENC_HALO_TOK, measured the
same way on the encoder, is recorded for a streaming sender, which does not exist yet.

``schedule`` is host arithmetic only; ``StreamReceiver`` is the session object (``ProposedEval.stream_receiver``).
"""
from __future__ import annotations

from typing import List, Tuple

HOP = 320                         # samples per latent token (the product of the decoder rates)
DEC_TAIL = 8                      # T_DEC(z[..., :T]) has 320*T - 8 samples
DEC_HALO_TOK = 10                 # tokens of context on each side of what a window may emit (3200 samples)
DEC_HALO_SAMPLES = (3132, 3141)   # inexact samples at the start / end of a window that is not at the sequence's edge
ENC_HALO_TOK = 8                  # the encoder's halo, each side (for the streaming sender: not built)
CHUNK_TOK = 16                    # proposed.AR_CHUNK_TOK, restated so that schedule() needs no torch


def schedule(T: int, chunk: int = CHUNK_TOK, halo: int = DEC_HALO_TOK) -> List[Tuple[int, int, int, int]]:
    """The steps of a session over T tokens: (win_start_tok, win_end_tok, emit_start, emit_end), tokens and global samples.

    One step per full chunk pushed, then the ``finish`` step (always the last entry; it takes the 0..chunk-1 remaining tokens).
    With N' tokens received before a push and N after it the window is [max(0, N' - 2*halo), N) and the step emits samples
    [320*(N' - halo), 320*(N - halo)) clamped at 0: every emitted sample lies ``halo`` tokens inside the window unless the window
    edge is the sequence's.  ``finish`` decodes [max(0, N' - 2*halo), T) and emits up to 320*T - 8.  Window lengths are 16, 32,
    then 36 tokens in the steady state (chunk 16, halo 10): 2.25 times the tokens emitted."""
    T, chunk, halo = int(T), int(chunk), int(halo)
    if T < 0 or chunk < 1 or halo < 0:
        raise ValueError(f"schedule: T={T}, chunk={chunk}, halo={halo}")
    steps, before = [], 0
    for n in range(chunk, T + 1, chunk):
        steps.append((max(0, before - 2 * halo), n, HOP * max(0, before - halo), HOP * max(0, n - halo)))
        before = n
    steps.append((max(0, before - 2 * halo), T, HOP * max(0, before - halo), max(0, HOP * T - DEC_TAIL)))
    return steps


class StreamReceiver:
    """A receiver session for ``batch`` items advancing in lockstep: ``push`` one 16-token chunk at a time (whatever tactile
    packets of it arrived, and its audio codes), get back the samples that chunk completes; ``finish`` flushes.

    ``cat(pushes + [finish])`` equals ``decompress_packets`` on the same packets bit for bit (length 320*T - 8), for
    ``ops.get_arith() == "f32"``: the opt-in arithmetic modes scale per item, so a window changes their arithmetic and no equality
    is claimed for them.  A push returns the samples up to 10 tokens (the decoder look-ahead) before the newest token, so the
    algorithmic latency is one chunk plus the halo, 213.3 + 133.3 ms, instead of the whole item.

    ``push`` runs, in order: packets.gather(seq_base=) per item -> ONE upload of the packet bodies and counts ->
    ops.idx_unpack_packets -> decode_latents(nb_valid=, z_prev=carry, z_last_out=carry) -> ops.stream_window (window = history
    | new latents; history updated in place) -> T_DEC on the window -> the emit slice (-> StreamResample for out_rate=3000).
    All session state is in fixed device buffers (carry [B, C], history [B, C, 20], the resampler's [B, 105]).

    ``graph=True``: the steady step (36-token window, from the third push on) is captured once as a graph on one stream and
    replayed for every later chunk after the host has written the packet bodies and audio codes into the static upload buffers;
    the first two pushes and ``finish`` run eagerly, and so does the resampler launch.  THE TENSOR A PUSH RETURNS IS THEN A VIEW OF
    THE GRAPH'S OUTPUT BUFFER: it is valid until the next push (clone it to keep it)."""

    def __init__(self, net, K, nb, packet_tok=2, batch=1, books_use=None, conceal="predict", out_rate=24000, graph=False):
        import torch
        from . import proposed
        from .packets import StreamInfo, body_bytes, _check
        K, nb, packet_tok, batch = int(K), int(nb), int(packet_tok), int(batch)
        if conceal == "plc":
            raise ValueError("StreamReceiver: conceal='plc' attends over the whole sequence and cannot run on a chunk")
        if conceal not in ("predict", "zero"):
            raise ValueError(f"StreamReceiver: conceal must be 'predict' or 'zero', not {conceal!r}")
        if packet_tok < 1 or CHUNK_TOK % packet_tok:
            raise ValueError(f"StreamReceiver: packet_tok = {packet_tok} does not divide the {CHUNK_TOK}-token chunk "
                             "(a packet must never straddle two chunks)")
        if K != net.vq.n_embed:
            raise ValueError(f"StreamReceiver: the stream has K = {K}, the model's codebook has {net.vq.n_embed}")
        if not 0 <= nb <= net.vq.n_books:
            raise ValueError(f"StreamReceiver: nb = {nb} books, the model has {net.vq.n_books}")
        if batch < 1:
            raise ValueError("StreamReceiver: batch must be at least 1")
        if int(out_rate) not in (proposed.EVAL_SR, proposed.ORIG_3K):
            raise ValueError(f"StreamReceiver: out_rate must be {proposed.EVAL_SR} or {proposed.ORIG_3K}, not {out_rate}")
        assert proposed.AR_CHUNK_TOK == CHUNK_TOK
        _check(StreamInfo(K, nb, CHUNK_TOK, packet_tok))
        self.net, self.K, self.nb, self.packet_tok, self.batch = net, K, nb, packet_tok, batch
        self.books_use, self.conceal, self.out_rate, self.graph = books_use, conceal, int(out_rate), bool(graph)
        self.dev = net.proj_up.weight.device
        self.C = net.proj_up.out_channels
        self.full = body_bytes(packet_tok, nb, K)
        self.carry = torch.zeros(batch, self.C, device=self.dev)                       # z_run[..., -1] of the chunk before
        self.hist = torch.zeros(batch, self.C, 2 * DEC_HALO_TOK, device=self.dev)      # the last <= 20 latent tokens
        self.h = 0                                                                     # valid columns of hist
        self.tokens = 0                                                                # tokens received (N)
        self.late = 0                                                                  # packets of chunks already decoded
        self.finished = False
        self.rs = None
        if self.out_rate != proposed.EVAL_SR:
            from .resample import StreamResample
            self.rs = StreamResample(proposed.EVAL_SR, self.out_rate, batch, device=self.dev)
        self._g = None                                                                 # (graph, up_static, codes_static, y_static)

    # ------------------------------------------------------------------------------------------------------------ stages
    def _gather(self, tactile_packets, n):
        """Host: per item whatever packets of this chunk arrived -> one uint8 array, bodies then counts."""
        import numpy as np
        from .packets import StreamInfo, gather
        info = StreamInfo(self.K, self.nb, n, self.packet_tok)
        B, P, full = self.batch, info.P, self.full
        host = np.empty(B * P * (full + 1), np.uint8)
        hb, hr = host[:B * P * full].reshape(B, P, full), host[B * P * full:].reshape(B, P)
        base, late = self.tokens // self.packet_tok, []
        for b in range(B):
            hb[b], hr[b] = gather(tactile_packets[b], info, seq_base=base, late=late)
        self.late += len(late)
        return host

    def _latents(self, up, codes, n):
        """Device: upload -> indices -> this chunk's latents [B, C, n]; the carried token moves on in place."""
        from . import ops
        B, full = self.batch, self.full
        P = (n + self.packet_tok - 1) // self.packet_tok
        idx, nbv = ops.idx_unpack_packets(up[:B * P * full].view(B, P, full), up[B * P * full:].view(B, P), self.K, self.nb, n,
                                          self.packet_tok)
        z = self.net.decode_latents(codes, idx, books_use=self.books_use, nb_valid=nbv, z_prev=self.carry, z_last_out=self.carry)
        if self.conceal == "zero":                            # the post-pass of decode_latents(conceal="zero"), after the carry
            z = ops.plc_mask_fill(z, None, nbv == 0)[0]
        return z

    def _window_decode(self, z, h_in, h_out, e0, e1):
        """Device: window = [history | z] (history updated in place), T_DEC on it, samples [e0, e1) of the window's output."""
        from . import ops
        win = ops.stream_window(self.hist, h_in, z, h_out)
        return self.net.T_DEC(win)[..., e0:e1]

    def _device_step(self, up, codes, n, h_in, h_out, e0, e1):
        return self._window_decode(self._latents(up, codes, n), h_in, h_out, e0, e1)

    def _plan(self, n, last):
        """(h_in, h_out, e0, e1) of the step that takes n new tokens: schedule()'s step in window-local samples."""
        before, after = self.tokens, self.tokens + n
        a = max(0, before - 2 * DEC_HALO_TOK)
        assert self.h == before - a
        g0 = HOP * max(0, before - DEC_HALO_TOK)
        g1 = max(0, HOP * after - DEC_TAIL) if last else HOP * max(0, after - DEC_HALO_TOK)
        return self.h, min(2 * DEC_HALO_TOK, self.h + n), g0 - HOP * a, g1 - HOP * a

    def _codes(self, audio_codes, n_lo, n_hi):
        import torch
        codes = torch.as_tensor(audio_codes)
        if codes.dim() != 3 or codes.shape[0] != self.batch or codes.dtype.is_floating_point or codes.dtype == torch.bool:
            raise ValueError(f"StreamReceiver: audio_codes must be int [B={self.batch}, n_codebooks, tokens], got {tuple(codes.shape)}")
        if codes.shape[1] != self.net.A_QUANT.n_codebooks:
            raise ValueError(f"StreamReceiver: {codes.shape[1]} audio code rows, the model's quantiser has {self.net.A_QUANT.n_codebooks}")
        if not n_lo <= codes.shape[2] <= n_hi:
            want = f"{n_lo}" if n_lo == n_hi else f"{n_lo}..{n_hi}"
            raise ValueError(f"StreamReceiver: {codes.shape[2]} audio tokens for a chunk of {want} tokens")
        return codes

    def _packets_ok(self, tactile_packets):
        tactile_packets = list(tactile_packets)
        if len(tactile_packets) != self.batch:
            raise ValueError(f"StreamReceiver: packets of {len(tactile_packets)} items for a session of batch {self.batch}")
        return tactile_packets

    def _out(self, y, last):
        if self.rs is None:
            return y
        return self.rs.finish(y) if last else self.rs.push(y)

    # ------------------------------------------------------------------------------------------------------------ session
    def push(self, tactile_packets, audio_codes):
        """One chunk: ``tactile_packets`` = ``batch`` iterables of the packets of chunk c that arrived (the stream's sequence
        numbers [c*16/packet_tok, (c+1)*16/packet_tok); missing, reordered, duplicated or thinned), ``audio_codes`` int [B, 32, 16].
        -> y [B, 1, n_emit] (1920 samples for the first push, then 5120; a third of that at out_rate=3000, less the resampler's
        look-ahead).  A packet of an earlier chunk is counted in ``late`` and ignored; one of a later chunk raises ValueError.
        With graph=True the result is valid until the next push."""
        import torch
        from ._lib import MvqError
        if self.finished:
            raise MvqError("StreamReceiver: push after finish")
        tactile_packets = self._packets_ok(tactile_packets)
        codes = self._codes(audio_codes, CHUNK_TOK, CHUNK_TOK)
        n = CHUNK_TOK
        host = self._gather(tactile_packets, n)
        plan = self._plan(n, False)
        with torch.no_grad():
            if self.graph and plan[0] == 2 * DEC_HALO_TOK:                    # the steady step: a full history
                y = self._replay(host, codes, n, plan)
            else:
                y = self._device_step(torch.from_numpy(host).to(self.dev), codes.to(self.dev), n, *plan)
            self.h, self.tokens = plan[1], self.tokens + n
            return self._out(y, False)

    def finish(self, tactile_packets=None, audio_codes=None):
        """Flush: optionally a last partial chunk of 1..15 tokens (its packets and audio_codes [B, 32, n]), then every remaining
        sample up to 320*T - 8.  Runs eagerly.  The session accepts nothing afterwards."""
        import torch
        from ._lib import MvqError
        if self.finished:
            raise MvqError("StreamReceiver: finish after finish")
        if (tactile_packets is None) != (audio_codes is None):
            raise ValueError("StreamReceiver.finish: the last chunk needs both its packets and its audio codes")
        n, host, codes = 0, None, None
        if audio_codes is not None:
            tactile_packets = self._packets_ok(tactile_packets)
            codes = self._codes(audio_codes, 1, CHUNK_TOK - 1)
            n = int(codes.shape[2])
            host = self._gather(tactile_packets, n)
        plan = self._plan(n, True)
        with torch.no_grad():
            if n:
                z = self._latents(torch.from_numpy(host).to(self.dev), codes.to(self.dev), n)
            else:
                z = torch.empty(self.batch, self.C, 0, device=self.dev)
            if self.h + n:
                y = self._window_decode(z, *plan)
            else:
                y = torch.empty(self.batch, 1, 0, device=self.dev)
            self.h, self.tokens, self.finished = plan[1], self.tokens + n, True
            return self._out(y, True)

    def _replay(self, host, codes, n, plan):
        """The steady step as a graph: captured at its first use (after one eager run at that shape on copies of the state, so
        that nothing is built during the capture), then replayed with the inputs written into the static buffers."""
        import torch
        if self._g is None:
            up_s = torch.from_numpy(host).to(self.dev)
            codes_s = codes.to(self.dev).long().clone()
            keep = (self.hist.clone(), self.carry.clone())
            g = torch.cuda.CUDAGraph()
            s = torch.cuda.Stream(device=self.dev)
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                self._device_step(up_s, codes_s, n, *plan)                   # warm-up at the steady shape; it moved the state on
                self.hist.copy_(keep[0])
                self.carry.copy_(keep[1])
                with torch.cuda.graph(g, stream=s):
                    y_s = self._device_step(up_s, codes_s, n, *plan)
            torch.cuda.current_stream().wait_stream(s)
            self._g = (g, up_s, codes_s, y_s)
        else:
            g, up_s, codes_s, y_s = self._g
            up_s.copy_(torch.from_numpy(host))
            codes_s.copy_(codes)
        g.replay()
        return y_s
