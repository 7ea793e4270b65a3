"""``Resample`` -- the ``torchaudio.transforms.Resample(orig_freq, new_freq)`` object the reference builds for every file
(``resample_to``: Training/compare_dacvsproposal_5.py:110-113; Evaluation/dac_vcpwq_proposed6_latency.py:151-156), default
arguments (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99), on libmvq_hip.so.

The filter bank is designed in float64 on the host exactly as torchaudio's ``_get_sinc_resample_kernel`` does and rounded
to fp32; the convolution is one HBM-bound launch (``mvq_resample_f32``).  torchaudio itself is not a dependency.
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn

from . import _lib, ops


def sinc_resample_kernel(orig_freq: int, new_freq: int, lowpass_filter_width: int = 6, rolloff: float = 0.99):
    """-> (kern[new, 2*width + orig] fp32, width, orig, new) with orig/new the rates divided by their gcd."""
    g = math.gcd(int(orig_freq), int(new_freq))
    orig, new = int(orig_freq) // g, int(new_freq) // g
    base = min(orig, new) * rolloff
    width = int(math.ceil(lowpass_filter_width * orig / base))
    idx = torch.arange(-width, width + orig, dtype=torch.float64).unsqueeze(0) / orig
    t = (torch.arange(0, -new, -1, dtype=torch.float64).unsqueeze(1) / new + idx) * base
    t = t.clamp(-lowpass_filter_width, lowpass_filter_width)
    window = torch.cos(t * math.pi / lowpass_filter_width / 2) ** 2
    t = t * math.pi
    kern = torch.where(t == 0, torch.ones_like(t), torch.sin(t) / t) * window * (base / orig)
    return kern.to(torch.float32).contiguous(), width, orig, new


class Resample(nn.Module):
    def __init__(self, orig_freq: int = 16000, new_freq: int = 16000, resampling_method: str = "sinc_interp_hann",
                 lowpass_filter_width: int = 6, rolloff: float = 0.99):
        super().__init__()
        if resampling_method != "sinc_interp_hann":
            raise ops.MvqError("Resample: only the default sinc_interp_hann method is built (what the reference uses)")
        self.orig_freq, self.new_freq = int(orig_freq), int(new_freq)
        kern, self.width, self.orig, self.new = sinc_resample_kernel(orig_freq, new_freq, lowpass_filter_width, rolloff)
        self.register_buffer("kernel", kern, persistent=False)

    @torch.no_grad()
    def forward(self, waveform: torch.Tensor) -> torch.Tensor:
        if self.orig_freq == self.new_freq:
            return waveform
        x = ops._dev(waveform.to(torch.float32).contiguous(), "waveform")
        lead, L = x.shape[:-1], x.shape[-1]
        B = x.numel() // max(L, 1) if L else 0
        Lout = int(math.ceil(self.new * L / self.orig))
        y = torch.empty(lead + (Lout,), device=x.device, dtype=torch.float32)
        kern = self.kernel if self.kernel.device == x.device else self.kernel.to(x.device)
        ops.check(_lib.lib().mvq_resample_f32(x.data_ptr(), kern.data_ptr(), y.data_ptr(), B, L, Lout, self.orig, self.new,
                                              self.width, kern.shape[1], ops._stream()), "mvq_resample_f32")
        return y


def resample_to(wav: torch.Tensor, sr_in: int, sr_out: int) -> torch.Tensor:
    """The reference's helper (Training/compare_dacvsproposal_5.py:110-113)."""
    if sr_in == sr_out:
        return wav
    return Resample(sr_in, sr_out).to(wav.device)(wav)


class StreamResample:
    """``Resample(orig_freq, new_freq)`` fed piece by piece for ``batch`` signals in lockstep (mvq_resample_stream_f32; pure
    decimation only: new_freq must divide orig_freq).  ``push(x[B, ..., n])`` returns the outputs that piece completes -- output n
    needs input sample n*orig + width + orig - 1 (8n + 56 for 24 kHz -> 3 kHz) -- and ``finish(x=None)`` pads on the right and
    flushes; a pushed piece must be a multiple of ``orig`` samples long, the final one need not.  The concatenated outputs equal
    ``Resample(orig_freq, new_freq)`` of the concatenated input bit for bit.  The state is one fixed device buffer
    [batch, ceil(width/orig)*orig + width] that the kernel updates in place."""

    def __init__(self, orig_freq: int, new_freq: int, batch: int, device=None, lowpass_filter_width: int = 6, rolloff: float = 0.99):
        kern, self.width, self.orig, self.new = sinc_resample_kernel(orig_freq, new_freq, lowpass_filter_width, rolloff)
        if self.new != 1:
            raise ops.MvqError(f"StreamResample: {orig_freq} -> {new_freq} Hz is no pure decimation (the streamed kernel covers new = 1)")
        self.orig_freq, self.new_freq, self.batch = int(orig_freq), int(new_freq), int(batch)
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.kernel = kern.to(device)
        self.state = ops.resample_stream_state(self.orig, self.width, self.batch, device)
        self.consumed, self.done, self._lead = 0, False, (self.batch,)

    def _piece(self, x, final):
        if self.done:
            raise ops.MvqError("StreamResample: the stream is finished")
        if x.shape[0] != self.batch or x.numel() != self.batch * x.shape[-1]:
            raise ops.MvqError(f"StreamResample: a piece must be [B={self.batch}, ..., n], got {tuple(x.shape)}")
        lead, n = tuple(x.shape[:-1]), x.shape[-1]
        self._lead = lead                                                    # finish() without a piece answers in this shape
        y = ops.resample_stream(x.reshape(self.batch, n), self.kernel, self.state, self.consumed, self.orig, self.new, self.width,
                                final=final)
        self.consumed += n
        self.done = final
        return y.reshape(lead + (y.shape[-1],))

    @torch.no_grad()
    def push(self, x: torch.Tensor) -> torch.Tensor:
        return self._piece(x, False)

    @torch.no_grad()
    def finish(self, x: torch.Tensor = None) -> torch.Tensor:
        if x is None:
            x = torch.empty(self._lead + (0,), device=self.state.device)
        return self._piece(x, True)


class StreamResampleRational:
    """``Resample(orig_freq, new_freq)`` fed piece by piece for ``batch`` signals in lockstep, for any ratio
    (mvq_resample_stream_rational_f32): ``StreamResample``'s contract with a polyphase bank.  With orig / new the rates divided by
    their gcd, a filter block is ``orig`` input samples and ``new`` outputs.  ``push(x[B, ..., n])`` returns the outputs that piece
    completes, ``hold`` blocks behind the input (None: ceil(width/orig), the smallest lag; a larger one aligns the pieces, e.g. with
    the 320-sample tokens of the native-rate sender); ``finish(x=None)`` pads on the right and flushes.  A pushed piece must be a
    multiple of ``orig`` samples long, the final one need not.  The concatenated outputs equal ``Resample(orig_freq, new_freq)`` of
    the concatenated input bit for bit.  The state is one fixed device buffer [batch, hold*orig + width] (at most 1024 samples) that
    the kernel updates in place.  ``form``: "block" (one block per signal) or "split" (ops.resample_stream_rational: the same
    results from the two-launch form, the faster one for few signals)."""

    def __init__(self, orig_freq: int, new_freq: int, batch: int, device=None, hold: int = None, lowpass_filter_width: int = 6,
                 rolloff: float = 0.99, form: str = "block"):
        if form not in ops.RESAMPLE_FORMS:
            raise ops.MvqError(f"StreamResampleRational: form must be 'block' or 'split', not {form!r}")
        self.form = form
        if int(orig_freq) == int(new_freq):
            raise ops.MvqError(f"StreamResampleRational: {orig_freq} -> {new_freq} Hz changes nothing (Resample returns its input)")
        kern, self.width, self.orig, self.new = sinc_resample_kernel(orig_freq, new_freq, lowpass_filter_width, rolloff)
        least = (self.width + self.orig - 1) // self.orig
        self.hold = least if hold is None else int(hold)
        if self.hold < least:
            raise ops.MvqError(f"StreamResampleRational: hold = {self.hold} blocks; {orig_freq} -> {new_freq} Hz needs at least {least}")
        if self.hold * self.orig + self.width > 1024:
            raise ops.MvqError(f"StreamResampleRational: a state of {self.hold * self.orig + self.width} samples "
                               f"(hold = {self.hold}) exceeds the kernel's 1024")
        self.orig_freq, self.new_freq, self.batch = int(orig_freq), int(new_freq), int(batch)
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.kernel = kern.to(device)
        self.state = ops.resample_stream_rational_state(self.orig, self.width, self.batch, device, self.hold)
        self.consumed, self.done, self._lead = 0, False, (self.batch,)

    def out_len(self, n: int, final: bool = False) -> int:
        """Outputs the next piece of ``n`` samples would complete."""
        from .stream import resample_stream_rational_out_len
        return resample_stream_rational_out_len(self.consumed, int(n), self.orig, self.new, self.width, self.hold, final)

    def _piece(self, x, final):
        if self.done:
            raise ops.MvqError("StreamResampleRational: the stream is finished")
        if x.shape[0] != self.batch or x.numel() != self.batch * x.shape[-1]:
            raise ops.MvqError(f"StreamResampleRational: a piece must be [B={self.batch}, ..., n], got {tuple(x.shape)}")
        lead, n = tuple(x.shape[:-1]), x.shape[-1]
        y = ops.resample_stream_rational(x.to(torch.float32).reshape(self.batch, n), self.kernel, self.state, self.consumed, self.orig,
                                         self.new, self.width, hold=self.hold, final=final, form=self.form)
        self._lead = lead                                                    # finish() without a piece answers in this shape
        self.consumed += n
        self.done = final
        return y.reshape(lead + (y.shape[-1],))

    @torch.no_grad()
    def push(self, x: torch.Tensor) -> torch.Tensor:
        return self._piece(x, False)

    @torch.no_grad()
    def finish(self, x: torch.Tensor = None) -> torch.Tensor:
        if x is None:
            x = torch.empty(self._lead + (0,), device=self.state.device)
        return self._piece(x, True)
