"""Streaming link, both ends.  Receiver: the tactile waveform chunk by chunk, bit-equal to the whole-item ``decompress_packets``
(DESIGN.md section 14).  Sender: packets and audio codes chunk by chunk, byte-equal to the whole-item ``compress_packets``
(section 15; ``sender_schedule``, ``StreamSender`` below).

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
extents are properties of the architecture (kernel sizes, dilations, strides), not of the weights.  ENC_HALO_TOK is measured the
same way on the encoder (oracle.dac_encoder, synth.dac_state(seed=7) encoder weights): encoding the samples of tokens [20, 55)
of a 75-token item reproduces the whole-item latents bit for bit except for the first 8 and the last 8 tokens of the window, and
a window that starts on a multiple of 320 samples keeps every stage's stride alignment, so a true sequence edge is exact
(tests/test_sender_cpu.py: the sender's schedule is exact at halo 8 and not at halo 7).

``StreamReceiver(decoder="stateful")`` replaces the latent window by a history PER DECODER STAGE: every stage
keeps the tail of its own input and a step computes it on [tail | new columns] only; ``decoder_stage_plan`` is that step's host
arithmetic (DEC_STAGES, DEC_STAGE_TAILS), and every call returns the window mode's tensor.

``StreamSender(encoder="stateful")`` does the same for the sender's 2x encoder window: every encoder stage keeps
the raw tail of its own input, ``encoder_stage_plan`` is a step's host arithmetic (ENC_STAGES, ENC_STAGE_TAILS) and
``sender_step_stateful`` the session's; every call returns the window mode's packets and codes.

``schedule`` / ``sender_schedule`` are host arithmetic only; ``StreamReceiver`` / ``StreamSender`` are the session objects
(``ProposedEval.stream_receiver`` / ``ProposedEval.stream_sender``).  ``StreamReceiverPool`` (``ProposedEval.stream_receiver_pool``)
serves receiver sessions that join, run and leave independently: their state lies in slots of one set of device buffers and a
tick batches whichever sessions have a chunk ready, grouped by ``pool_groups``.  ``StreamSenderPool``
(``ProposedEval.stream_sender_pool``) is the same for sender sessions, which push 1..16 tokens of samples at a time: ``sender_step``
is a session's host arithmetic, ``sender_pool_groups`` the sessions of a tick that share an encode.
``StreamSenderPoolAV`` / ``StreamReceiverPoolAV`` (``ProposedEval.stream_sender_pool_av`` / ``stream_receiver_pool_av``) are the two
pools with every option of the lockstep sessions -- rate control, audio packets, FEC on both streams, audio concealment: the same
sessions and groups.  ``_RxFront`` is every receiver's front end -- the whole-item calls', the lockstep
session's and the pools': it owns the format of the upload (``receiver_layout``), fills it on the host and unpacks it on the device.
``_TxBack`` is its mirror, every sender's back end: it owns the format of the read-back, packs it on the device and frames it on
the host.  ``_SessionTable`` is the session bookkeeping the four pools share.

``audio_out_rate=`` hands the receiver's audio output out at the playback rate: ``native_out_plan`` is its host
arithmetic and its refusals, ``_ReceiverCore._audio_rate`` the resample launch behind the fade, ``audio_resample_form`` the choice
between the one-block and the split form of the rational streamed resampler.
"""
from __future__ import annotations

import functools
from typing import List, NamedTuple, Tuple

HOP = 320                         # samples per latent token (the product of the decoder rates)
LINK_SR = 24000                   # proposed.EVAL_SR, the rate both encoders run at, restated so that the host arithmetic needs no torch
DEC_TAIL = 8                      # T_DEC(z[..., :T]) has 320*T - 8 samples
DEC_HALO_TOK = 10                 # tokens of context on each side of what a window may emit (3200 samples)
DEC_HALO_SAMPLES = (3132, 3141)   # inexact samples at the start / end of a window that is not at the sequence's edge
ENC_HALO_TOK = 8                  # the encoder's halo, each side (the streaming sender's look-back and look-ahead)
CHUNK_TOK = 16                    # proposed.AR_CHUNK_TOK, restated so that schedule() needs no torch
PUSH_MAX_TOK = 16                 # a sender push carries 1..16 tokens of samples, so it completes at most one chunk
SEND_CAP_TOK = 48                 # the sender's sample buffer: it never holds more than 47 tokens of samples
ENC_RATES = (2, 4, 5, 8)          # dac.ENC_RATES, restated so that sender_schedule() needs no torch
RS_ORIG, RS_WIDTH = 8, 49         # resample.sinc_resample_kernel(24000, 3000): decimation and filter half-width, restated likewise


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


def enc_tokens(samples: int, rates=ENC_RATES) -> int:
    """Latent tokens the encoder stack makes of ``samples`` samples (per stage a conv of kernel 2s, stride s, padding ceil(s/2))."""
    n = int(samples)
    for r in rates:
        n = (n + 2 * ((r + 1) // 2) - 2 * r) // r + 1 if n > 0 else 0
    return max(0, n)


def sender_schedule(T_tokens: int, pushes, chunk: int = CHUNK_TOK, halo: int = ENC_HALO_TOK) -> List[Tuple[int, int, int, int, int]]:
    """The steps of a sender session over an item of T_tokens tokens fed in ``pushes`` (tokens of samples per push, each
    1..PUSH_MAX_TOK, sum <= T_tokens; whatever remains goes to ``finish``): one entry per push and then the ``finish`` entry,
    each (win_start_tok, win_end_tok, chunk_first, chunk_end, held_tok) -- the encoder window in tokens (empty when nothing is
    emitted), the chunks [chunk_first, chunk_end) the step emits, and the tokens of samples the session holds afterwards.

    Chunk c (tokens [16c, 16c+16)) leaves with the push after which 16c + 16 + halo tokens are in hand: one chunk plus the
    look-ahead, 213.3 + 106.7 ms.  Its window is [max(0, 16c - halo), 16c + 16 + halo): 24 tokens for chunk 0, then 32 in the
    steady state, 2 times the tokens emitted (the receiver's decoder windows: 2.25 times).  After the emit the session keeps
    the samples from token 16c + 16 - halo on.  A push of at most 16 tokens completes at most one chunk: before it fewer than
    16(c+1) + halo tokens are in hand, after it fewer than 16(c+2) + halo.  ``finish`` encodes [max(0, 16c - halo), T) once and
    emits every remaining chunk; the window's right edge is the item's, which is exact."""
    T, chunk, halo = int(T_tokens), int(chunk), int(halo)
    pushes = [int(m) for m in pushes]
    if T < 0 or chunk < 1 or halo < 0 or chunk > PUSH_MAX_TOK:
        raise ValueError(f"sender_schedule: T={T}, chunk={chunk}, halo={halo}")
    if any(not 1 <= m <= PUSH_MAX_TOK for m in pushes) or sum(pushes) > T:
        raise ValueError(f"sender_schedule: pushes of 1..{PUSH_MAX_TOK} tokens that sum to at most T = {T}")
    steps, have, c, start = [], 0, 0, 0                                  # tokens in hand, next chunk, first token held
    for m in pushes:
        have += m
        if have >= chunk * (c + 1) + halo:
            steps.append((start, chunk * (c + 1) + halo, c, c + 1, have - max(0, chunk * (c + 1) - halo)))
            c, start = c + 1, max(0, chunk * (c + 1) - halo)
        else:
            steps.append((start, start, c, c, have - start))
    n_chunks = (T + chunk - 1) // chunk
    steps.append((start, T, c, n_chunks, 0) if n_chunks > c else (start, start, c, c, 0))
    return steps


def _window_plan(before: int, n: int, last: bool) -> Tuple[int, int, int, int]:
    """(h_in, h_out, e0, e1) of the step that takes n new tokens after ``before``: schedule()'s step in window-local samples."""
    a = max(0, before - 2 * DEC_HALO_TOK)
    h = before - a
    g0 = HOP * max(0, before - DEC_HALO_TOK)
    g1 = max(0, HOP * (before + n) - DEC_TAIL) if last else HOP * max(0, before + n - DEC_HALO_TOK)
    return h, min(2 * DEC_HALO_TOK, h + n), g0 - HOP * a, g1 - HOP * a


DEC_RATES = (8, 5, 4, 2)          # dac.DEC_RATES, restated so that decoder_stage_plan() needs no torch
DEC_RU_LOSS = 3 * (1 + 3 + 9)     # columns the three ResidualUnits (k7, dilations 1, 3, 9) lose at a cut edge


def _dec_stage_geometry(rates=DEC_RATES):
    """The decoder's stages as (stride s, off, loss): a window of w > 0 input columns makes w*s + off output columns, of which
    ``loss`` at every edge that is not the sequence's are inexact.  model.0 and the final conv are k7 (s = 1, loss 3); a
    DecoderBlock is a transposed conv (kernel 2s, padding p = ceil(s/2): off = s - 2p, it loses s - p columns) and three units."""
    blocks = tuple((s, s - 2 * ((s + 1) // 2), s - (s + 1) // 2 + DEC_RU_LOSS) for s in rates)
    return ((1, 0, 3),) + blocks + ((1, 0, 3),)


DEC_STAGES = _dec_stage_geometry()
# Tail columns a stage keeps of its own input.  The least that is exact: ceil((2*loss - off) / s) -- the
# next window's first exact output column must not lie past the last one already handed on -- 6, 11, 17, 21, 40; the final conv
# also holds back the samples between the stateful right edge (320*N - 3141) and the schedule's (320*(N - 10)) and needs 65.
# Each is rounded up to a multiple of 4, so that the steady windows (24, 28, 148, 664, 2600, 5188 columns) are too.
DEC_STAGE_TAILS = (8, 12, 20, 24, 40, 68)


class StageStep(NamedTuple):
    """One stage of one step: the window is [h_in tail columns | the producer's output columns [src_off, src_off + n_new)], and
    the last ``h_out`` columns of it are the tail afterwards."""
    h_in: int
    src_off: int
    n_new: int
    h_out: int


class StagePlan(NamedTuple):
    """``stages``: model.0, the four DecoderBlocks, the final conv; [e0, e1): the emitted samples, local to the final conv's output."""
    stages: Tuple[StageStep, ...]
    e0: int
    e1: int


def dec_stage_min_tails() -> Tuple[int, ...]:
    """The least tail every stage may keep: the first exact output column of the next window, (have - h)*s + loss, must not lie
    past the last column handed on, have*s + off - loss; the final conv must also reach back to the schedule's emit border,
    320*(N - 10), from its input's 320*N - 3138 columns."""
    need = [-(-(2 * loss - off) // s) for s, off, loss in DEC_STAGES]
    hop, add = 1, 0
    for s, off, loss in DEC_STAGES[:-1]:
        hop, add = hop * s, add * s + off - loss
    assert hop == HOP and hop * DEC_HALO_TOK + add >= DEC_STAGES[-1][2]         # the schedule's right margin covers the stack's loss
    need[-1] = max(need[-1], hop * DEC_HALO_TOK + add + DEC_STAGES[-1][2])
    return tuple(need)


assert dec_stage_min_tails() == (6, 11, 17, 21, 40, 65)
assert all(t >= m and t % 4 == 0 and t - m < 4 for t, m in zip(DEC_STAGE_TAILS, dec_stage_min_tails()))


def _dec_stage_have(tokens: int) -> List[int]:
    """Input columns every stage has received once ``tokens`` tokens went through pushes: what its producer could hand on, every
    window's right edge being cut (w*s + off - loss of its columns so far)."""
    have, x = [], int(tokens)
    for s, off, loss in DEC_STAGES:
        have.append(x)
        x = max(0, x * s + off - loss) if x > 0 else 0
    return have


def decoder_stage_plan(tokens_before: int, n: int, last: bool = False, tails=DEC_STAGE_TAILS) -> StagePlan:
    """The stateful decoder's step that takes ``n`` new tokens after ``tokens_before`` (host arithmetic; the library's
    mvq_decoder_stream_plan says the same).  Stage k's window covers its global input columns [a, b), a = have - h_in; its output
    column j is global column a*s + j.  Exact outputs: all of the window's, less ``loss`` at the left unless a == 0 and at the
    right unless ``last``.  What is handed on is what is exact and was not handed on before.  ``last`` flushes every stage against
    its true right edge (n = 0 too: the tails alone) and keeps nothing.  The emitted samples are stream.schedule's.  The plan
    depends on tokens_before only through min(tokens_before, 16): from 16 tokens on every tail is full.  ``tails`` other than
    DEC_STAGE_TAILS are for the tests: a tail below dec_stage_min_tails() hands on inexact columns."""
    before, n, last = int(tokens_before), int(n), bool(last)
    if before < 0 or n < 0:
        raise ValueError(f"decoder_stage_plan: tokens_before = {before}, n = {n}")
    have = _dec_stage_have(before)
    stages, src_off, n_new, a, hi = [], 0, n, 0, 0
    for (s, off, loss), cap, hv in zip(DEC_STAGES, tails, have):
        h_in = min(cap, hv)
        a, w = hv - h_in, h_in + n_new
        stages.append(StageStep(h_in, src_off, n_new, 0 if last else min(cap, w)))
        done = (max(0, hv * s + off - loss) if hv > 0 else 0) - a * s      # handed on before, local to this window's output
        hi = max(done, (w * s + off if w > 0 else 0) - (0 if last else loss))
        src_off, n_new = done, hi - done
    g0 = HOP * max(0, before - DEC_HALO_TOK)                               # the final conv has s = 1: its output column j is sample a + j
    g1 = max(0, HOP * (before + n) - DEC_TAIL) if last else HOP * max(0, before + n - DEC_HALO_TOK)
    if g1 <= g0:
        return StagePlan(tuple(stages), 0, 0)
    assert g0 >= a and g1 - a <= hi
    return StagePlan(tuple(stages), g0 - a, g1 - a)


ENC_RU_LOSS = DEC_RU_LOSS         # an EncoderBlock's three units lose the same 39 columns at a cut edge


def _enc_stage_geometry(rates=ENC_RATES):
    """The encoder's stages as (stride s, kernel ks, padding p, loss): output column J of a stage reads its input columns
    [J*s - p, J*s - p + ks) -- after ``loss`` columns were lost at every cut edge in front of the conv.  block.0 is k7 (padding 3),
    an EncoderBlock three units (loss 39) and a conv of kernel 2s, stride s, padding ceil(s/2), the last stage Snake + k3."""
    return ((1, 7, 3, 0),) + tuple((s, 2 * s, (s + 1) // 2, ENC_RU_LOSS) for s in rates) + ((1, 3, 1, 0),)


ENC_STAGES = _enc_stage_geometry()
# Tail columns a stage keeps of its own (raw) input: enc_stage_min_tails() rounded up to a multiple of 4.
ENC_STAGE_TAILS = (8, 84, 88, 92, 100, 4)
ENC_STREAM_MAX_N = (1 << 20) - 256   # samples of one step: every stage window stays within the stage-window kernel's 2^20 columns


def _enc_done(have: int, s: int, ks: int, p: int, loss: int) -> int:
    """Output columns of ``have`` input columns that are exact while the right edge is cut: J*s - p + ks <= have - loss."""
    x = have - loss + p - ks
    return x // s + 1 if x >= 0 else 0


def _enc_total(have: int, s: int, ks: int, p: int) -> int:
    """Output columns of ``have`` input columns whose right edge is the signal's (the conv's own length)."""
    x = have + 2 * p - ks
    return x // s + 1 if have > 0 and x >= 0 else 0


def _enc_tail(have: int, s: int, cap: int) -> int:
    """Rule 1: the tail actually used, the largest h <= min(cap, have) with (have - h) % s == 0 -- the window then starts on a
    global column that is a multiple of the stride."""
    return have if have <= cap else have - -(-(have - cap) // s) * s


def enc_stage_min_tails() -> Tuple[int, ...]:
    """The least tail every stage may keep for ANY number of input columns.  With d outputs handed on (the largest d with
    d*s - p + ks <= have - loss) the next window must start at a multiple of s at or below d*s - p - loss, its first new output
    column's left-most exact input; the largest such start is d*s - s*ceil((p + loss)/s), and have - d*s is at most
    loss - p + ks - 1.  77 + 2s plus the alignment slack for a block, 6 for k7, 2 for k3."""
    return tuple(loss - p + ks - 1 + s * -(-(p + loss) // s) for s, ks, p, loss in ENC_STAGES)


assert enc_stage_min_tails() == (6, 81, 88, 90, 98, 2)
assert all(t >= m and t % 4 == 0 and t - m < 4 for t, m in zip(ENC_STAGE_TAILS, enc_stage_min_tails()))


class EncStagePlan(NamedTuple):
    """``stages``: block.0, the four EncoderBlocks, the Snake + k3; [t0, t1): the GLOBAL latent columns (tokens) the step emits,
    ``off`` their first column local to the k3 window's output."""
    stages: Tuple[StageStep, ...]
    t0: int
    t1: int
    off: int


def encoder_stage_plan(samples_before: int, n: int, last: bool = False, tails=ENC_STAGE_TAILS, align: bool = True) -> EncStagePlan:
    """The stateful encoder's step that takes ``n`` new samples after ``samples_before`` (host arithmetic; the library's
    mvq_encoder_stream_plan says the same).  Stage k has received ``have`` columns; its window is [h_in tail columns | n_new new
    ones], h_in by rule 1 (_enc_tail), so it covers global input columns [a, have + n_new) with a % s == 0 and its output column j
    is global column a/s + j.  Rule 2: global output column J is exact if J*s - p >= a + loss (or a == 0) and J*s - p + ks <=
    have + n_new - loss (or ``last``: the true right edge).  What is handed on is what is exact and was not handed on before, so a
    stage's ``have`` is a function of samples_before alone.  ``last`` flushes every stage against its true right edge (n = 0 too:
    the tails alone) and keeps nothing.  ``tails`` other than ENC_STAGE_TAILS and ``align`` = False (the plain tail min(cap, have),
    a window start off the stride grid) are for the tests: both hand on inexact columns."""
    before, n, last = int(samples_before), int(n), bool(last)
    if before < 0 or n < 0 or n > ENC_STREAM_MAX_N:
        raise ValueError(f"encoder_stage_plan: samples_before = {before}, n = {n}")
    stages, have, src_off, n_new, d0, d1, off = [], before, 0, n, 0, 0, 0
    for (s, ks, p, loss), cap in zip(ENC_STAGES, tails):
        tail = (lambda hv: _enc_tail(hv, s, cap)) if align else (lambda hv: min(hv, cap))
        h_in = tail(have)
        a = have - h_in
        stages.append(StageStep(h_in, src_off, n_new, 0 if last else tail(have + n_new)))
        d0 = _enc_done(have, s, ks, p, loss)
        d1 = max(d0, _enc_total(have + n_new, s, ks, p) if last else _enc_done(have + n_new, s, ks, p, loss))
        off = d0 - a // s if d1 > d0 else 0
        if tails is ENC_STAGE_TAILS and align and d1 > d0:
            assert off >= 0 and (a == 0 or d0 * s - p - loss >= a)
        have, src_off, n_new = d0, off, d1 - d0
    return EncStagePlan(tuple(stages), d0, d1, off)


def resample_stream_out_len(consumed: int, n_new: int, orig: int, width: int, final: bool = False) -> int:
    """Outputs a resample_stream call completes after ``consumed`` samples: the count mvq_resample_stream_f32 checks."""
    hold = (width + orig - 1) // orig
    done = max(0, consumed // orig - hold)
    upto = -(-(consumed + n_new) // orig) if final else (consumed + n_new) // orig - hold
    return max(0, upto - done)


def resample_stream_rational_out_len(consumed: int, n_new: int, orig: int, new: int, width: int, hold: int = None,
                                     final: bool = False) -> int:
    """Outputs a resample_stream_rational call completes after ``consumed`` samples: the count mvq_resample_stream_rational_f32
    checks.  ``hold`` (None: ceil(width/orig)) is the lag in filter blocks of ``orig`` inputs / ``new`` outputs; a final call counts
    outputs up to ceil(new*(consumed + n_new)/orig).  With new == 1 and the default hold this is resample_stream_out_len."""
    hold = (width + orig - 1) // orig if hold is None else hold
    done = max(0, consumed // orig - hold)
    if final:
        return max(0, -(-new * (consumed + n_new) // orig) - new * done)
    return new * max(0, (consumed + n_new) // orig - hold - done)


def native_token_plan(in_rate: int, out_rate: int = 24000, hop: int = HOP, lowpass_filter_width: int = 6, rolloff: float = 0.99):
    """The native-rate sender's arithmetic of one modality -> (orig, new, width, hold, samples per token, state length): ``hold`` =
    the filter blocks of one ``hop``-sample token at ``out_rate``, so a resample call completes whole tokens.  ValueError when a
    token is no whole number of blocks (hop*orig % new), when one token of blocks is less than the filter needs, or when the state
    hold*orig + width exceeds the kernel's 1024 samples.  (width: resample.sinc_resample_kernel's, restated so that no torch is needed.)"""
    import math
    g = math.gcd(int(in_rate), int(out_rate))
    orig, new = int(in_rate) // g, int(out_rate) // g
    width = int(math.ceil(lowpass_filter_width * orig / (min(orig, new) * rolloff)))
    if hop * orig % new:
        raise ValueError(f"StreamSenderNative: at {in_rate} Hz a {hop}-sample token at {out_rate} Hz is {hop * orig}/{new} input "
                         "samples, no whole number of filter blocks")
    hold = hop // new                                                    # blocks per token (orig and new are coprime)
    if hold < (width + orig - 1) // orig:
        raise ValueError(f"StreamSenderNative: at {in_rate} Hz one token is {hold} filter blocks, fewer than the filter's "
                         f"{(width + orig - 1) // orig}")
    state = hold * orig + width
    if state > 1024:
        raise ValueError(f"StreamSenderNative: at {in_rate} Hz the resampler state is {state} samples; the kernel carries at most 1024")
    return orig, new, width, hold, hold * orig, state


def native_out_plan(who: str, audio_out_rate: int, audio_out: bool = True, hop: int = HOP, lowpass_filter_width: int = 6,
                    rolloff: float = 0.99):
    """The receiver's audio output at ``audio_out_rate`` Hz -> None at LINK_SR (nothing is resampled), else
    (orig, new, width, hold, state length) of the streamed resampler LINK_SR -> audio_out_rate at the smallest lag, hold =
    ceil(width/orig).  ValueError, with the caller's name ``who`` in front and the rate in the message, for a rate without
    audio_out=True, a rate at which a ``hop``-sample token is no whole number of filter blocks (hop % orig: every piece a session
    emits but its last is whole tokens, and only whole blocks can be pushed), and a state beyond the kernel's 1024 samples.  Every
    surface that takes audio_out_rate= calls this before it allocates anything."""
    import math
    rate = int(audio_out_rate)
    if rate == LINK_SR:
        return None
    if rate <= 0:
        raise ValueError(f"{who}: audio_out_rate = {audio_out_rate!r} Hz")
    if not audio_out:
        raise ValueError(f"{who}: audio_out_rate = {rate} Hz shapes the audio output; it goes with audio_out=True")
    g = math.gcd(LINK_SR, rate)
    orig, new = LINK_SR // g, rate // g
    if hop % orig:
        raise ValueError(f"{who}: audio_out_rate = {rate} Hz is {orig} : {new} against {LINK_SR} Hz, and a {hop}-sample token is no whole "
                         f"number of {orig}-sample filter blocks")
    width = int(math.ceil(lowpass_filter_width * orig / (min(orig, new) * rolloff)))
    hold = (width + orig - 1) // orig
    state = hold * orig + width
    if state > 1024:
        raise ValueError(f"{who}: audio_out_rate = {rate} Hz needs a resampler state of {state} samples; the kernel carries at most 1024")
    return orig, new, width, hold, state


# Which form of the rational streamed resampler the receiver's audio output takes, from the sessions of the launch (a lockstep
# session's batch, a pool group's size).  Set from tools/native_out_bench.py's same-run comparison:
# the steady 16-token piece, one block per session against split, medians of three alternating runs in ms on one MI355X --
#   24000 -> 44100:  B = 1  0.311 / 0.026    B = 6  0.313 / 0.026    B = 256  0.314 / 0.164   (the one-block form's spread: 0.002 - 0.004)
#   24000 -> 48000:  B = 1  0.069 / 0.025    B = 6  0.074 / 0.025    B = 256  0.078 / 0.038   (spread 0.001)
# The split form wins at every count measured, so no count up to 256 selects the one-block form; beyond 256 nothing is measured
# and the bound stays open until a measurement closes it.
AUDIO_RESAMPLE_SPLIT_MAX = 1 << 30


def audio_resample_form(sessions: int) -> str:
    """"split" for up to AUDIO_RESAMPLE_SPLIT_MAX sessions in a launch, else "block"."""
    return "split" if int(sessions) <= AUDIO_RESAMPLE_SPLIT_MAX else "block"


class PoolGroup(NamedTuple):
    """Sessions of one tick that share a launch sequence: ``key`` = (min(tokens_before, 32), n, last); ``sids`` ascending;
    ``plan`` = StreamReceiver._plan's (h_in, h_out, e0, e1) of every member; ``consumed`` = the resampler's launch class (the
    samples a member at the key's token count has emitted) and ``n_out`` the outputs its piece of e1 - e0 samples completes."""
    key: Tuple[int, int, bool]
    sids: Tuple[int, ...]
    plan: Tuple[int, int, int, int]
    consumed: int
    n_out: int


def pool_groups(sessions, orig: int = RS_ORIG, width: int = RS_WIDTH) -> List[PoolGroup]:
    """``sessions``: (sid, tokens_before, n, last) of every session that takes a step this tick -- a push has n = 16 and last
    False, a finish 0 <= n <= 15 and last True; tokens_before is a multiple of 16.  -> the groups, ordered by key.

    Sessions may share a launch sequence only when their launch parameters agree: the window plan (h_in, h_out, e0, e1) and the
    resampler's base, lead and output count.  All of them depend on tokens_before only through min(tokens_before, 32): the plan is
    that of 0, 16 or "32 and more" tokens (a full 20-token history, the emit range a fixed offset into the window), and the
    resampler has consumed 0 samples, 1920 or at least 7040 -- zero or beyond its 105-sample state, where base = 0 and lead = 0
    and the output count depends on the piece alone.  Nothing coarser is sound: sessions of different phases are never merged by
    padding, a zero-latent history is not the sequence edge."""
    seen, by_key = set(), {}
    for sid, before, n, last in sessions:
        before, n, last = int(before), int(n), bool(last)
        if sid in seen:
            raise ValueError(f"pool_groups: session {sid} is listed twice")
        seen.add(sid)
        if before < 0 or before % CHUNK_TOK or (n != CHUNK_TOK if not last else not 0 <= n < CHUNK_TOK):
            raise ValueError(f"pool_groups: session {sid}: tokens_before = {before}, n = {n}, last = {last}")
        by_key.setdefault((min(before, 2 * CHUNK_TOK), n, last), []).append(sid)
    out = []
    for key in sorted(by_key):
        before, n, last = key
        plan = _window_plan(before, n, last)
        consumed = HOP * max(0, before - DEC_HALO_TOK)
        n_out = resample_stream_out_len(consumed, plan[3] - plan[2], orig, width, last)
        out.append(PoolGroup(key, tuple(sorted(by_key[key])), plan, consumed, n_out))
    return out


class RxLayout(NamedTuple):
    """Byte offsets of a group's upload (``receiver_layout``); an absent part has offset None.  ``fec`` / ``audio_fec``: (rows, got)."""
    P: int
    bodies: int
    counts: int
    abodies: object
    acounts: object
    fec: object
    audio_fec: object
    size: int


def receiver_layout(G: int, n: int, full: int, afull, fec, audio_fec, packet_tok: int) -> RxLayout:
    """The layout of what a receiver uploads for ``G`` items of ``n`` tokens (host arithmetic; ``_RxFront`` is its one user and
    every receiver goes through that -- G = the batch of a whole-item call or a lockstep session, or a pool group's sessions):
    the tactile bodies uint8 [G, P, full], their counts [G, P]; with ``afull`` not None (audio packets) the audio bodies
    [G, P, afull] and their counts [G, P]; then per stream with a Fec -- ``fec`` / ``audio_fec`` = (group g, parity r, width W) as
    Fec.resolve gives them for the stream, or None -- its parity rows [G, Gr, r*(g + W)], Gr = ceil(P / g), then ``got`` [G, Gr]."""
    G, n, full, packet_tok = int(G), int(n), int(full), int(packet_tok)
    P = (n + packet_tok - 1) // packet_tok
    o = G * P * (full + 1)
    ab = ac = None
    if afull is not None:
        ab, ac = o, o + G * P * int(afull)
        o += G * P * (int(afull) + 1)
    at = []
    for f in (fec, audio_fec):
        if f is None:
            at.append(None)
            continue
        g, r, W = (int(v) for v in f)
        nr = G * ((P + g - 1) // g) * r * (g + W)
        at.append((o, o + nr))
        o += nr + G * ((P + g - 1) // g)
    return RxLayout(P, 0, G * P * full, ab, ac, at[0], at[1], o)


class _Streams:
    """What both ends of the link know of its streams: the tactile one (``K``, ``nb``, ``fec``) and, with ``audio`` = (K_a, na), the
    audio one (``audio_fec``); one ``packet_tok`` serves both."""

    def __init__(self, K, nb, packet_tok, audio=None, fec=None, audio_fec=None):
        from .packets import body_bytes
        self.K, self.nb, self.packet_tok, self.audio, self.fec, self.audio_fec = K, nb, packet_tok, audio, fec, audio_fec
        self.full = body_bytes(packet_tok, nb, K)
        self.afull = None if audio is None else body_bytes(packet_tok, audio[1], audio[0])
        self._streams = functools.lru_cache(None)(self._streams)          # a pure function of n; a session asks with every chunk

    def _streams(self, n):
        """(StreamInfo of ``n`` tokens, Fec or None) per stream: tactile, then audio."""
        from .packets import StreamInfo
        out = ((StreamInfo(self.K, self.nb, n, self.packet_tok), self.fec),)
        return out if self.audio is None else out + ((StreamInfo(*self.audio, n, self.packet_tok), self.audio_fec),)


class _RxFront(_Streams):
    """THE receiver front end, from "the packets that arrived" to indices and per-token counts on the device: the owner of the
    upload's format.  decompress_packets / decompress_packets_av, StreamReceiver and both receiver pools
    build their upload and read it through this object and hold no offset of their own.  The streams are ``_Streams``'."""

    def __init__(self, K, nb, packet_tok, audio=None, fec=None, audio_fec=None):
        from .packets import gather, gather_fec
        super().__init__(K, nb, packet_tok, audio, fec, audio_fec)
        self._gather, self._gather_fec = gather, gather_fec
        # pure functions of (G, n) and the layout, and a session asks for the same ones with every chunk: computed once each
        self.layout, self._spans = (functools.lru_cache(None)(f) for f in (self.layout, self._spans))

    def layout(self, G, n) -> RxLayout:
        """receiver_layout of ``G`` items of ``n`` tokens for these streams, every Fec resolved against its stream."""
        code = [None if f is None else (f.resolve(inf)[0], f.r, f.resolve(inf)[3]) for inf, f in self._streams(n)] + [None]
        return receiver_layout(G, n, self.full, self.afull, code[0], code[1], self.packet_tok)

    @staticmethod
    def _spans(lay):
        """[start, end) of every part of a segment, in layout order: the one place that turns an RxLayout into slices."""
        starts = [lay.bodies, lay.counts] + ([lay.abodies, lay.acounts] if lay.abodies is not None else [])
        starts += [o for at in (lay.fec, lay.audio_fec) if at is not None for o in at]
        return tuple(zip(starts, starts[1:] + [lay.size]))

    def gather_item(self, tactile, audio, fec_pk, audio_fec_pk, n, seq_base=0, late=None):
        """Host: whatever packets of ONE item's ``n`` tokens arrived -> its arrays in layout order: packets.gather per stream,
        then packets.gather_fec per stream with a Fec (None: no parity packet arrived).  ``seq_base`` / ``late`` as packets.gather
        takes them; a stream's groups are numbered from seq_base // fec.group."""
        streams, parts = self._streams(n), []
        for (inf, _), pk in zip(streams, (tactile, audio)):
            parts += self._gather(pk, inf, seq_base, late)
        for (inf, f), pk in zip(streams, (fec_pk, audio_fec_pk)):
            if f is not None:
                parts += self._gather_fec(() if pk is None else pk, inf, f, seq_base // int(f.group), late)
        return parts

    def fill(self, seg, lay, i, parts):
        """Host: item ``i``'s ``parts`` (gather_item's) into ``seg``, the uint8 segment of a group laid out by ``lay``: every
        part of the segment is [G, bytes of one item]."""
        for (at, _), part in zip(self._spans(lay), parts):
            at += i * part.size
            seg[at:at + part.size] = part.reshape(-1)

    def unpack(self, up, lay, G, n):
        """Device: views of the uploaded segment ``up`` by ``lay``, then per stream ops.fec_recover in place and
        ops.idx_unpack_packets -- recover tactile, unpack tactile, recover audio, unpack audio, the order inside the captured
        steady step -> (idx [nb, G, n], nb_valid [G, n], audio codes [G, na, n] or None, na_valid [G, n] or None)."""
        from . import ops
        streams = self._streams(n)
        part = iter([up[a:b] for a, b in self._spans(lay)])               # consumed in layout order: data parts, then parity parts
        data = [(next(part).view(G, lay.P, full), next(part).view(G, lay.P)) for _, full in zip(streams, (self.full, self.afull))]
        out = []
        for (inf, f), (bodies, counts) in zip(streams, data):
            if f is not None:
                shape = f.rows_shape(inf)
                ops.fec_recover(bodies, counts, next(part).view(G, *shape), next(part).view(G, shape[0]), inf, f)
            out += ops.idx_unpack_packets(bodies, counts, inf.K, inf.nb, n, self.packet_tok)
        if self.audio is None:
            return out[0], out[1], None, None
        return out[0], out[1], out[2].permute(1, 0, 2).contiguous(), out[3]   # [na, G, n] -> [G, na, n], on the device


class _TxBack(_Streams):
    """THE sender back end, the mirror of ``_RxFront``: from indices and per-packet counts on the device to framed packets on the
    host, and the owner of the read-back's format.  compress_packets / compress_packets_av, StreamSender
    and both sender pools pack their read-back and frame it through this object and hold no offset of their own.  ``counts``: the
    per-packet book counts ride behind each stream's bodies -- under a ``rate``, and always with audio packets."""

    def __init__(self, K, nb, packet_tok, audio=None, counts=False, fec=None, audio_fec=None):
        super().__init__(K, nb, packet_tok, audio, fec, audio_fec)
        self.counts = bool(counts) or audio is not None
        self.layout = functools.lru_cache(None)(self.layout)

    def layout(self, n):
        """The [start, end) bytes of every part of ONE item's row for ``n`` tokens, in the row's order: per stream (tactile, then
        audio) the bodies [P, full] and, with ``counts``, the counts [P]; then per stream with a Fec its parity rows
        (Fec.rows_shape).  The one place that turns the options into slices."""
        import itertools
        import math
        streams, sizes = self._streams(n), []
        for (inf, _), full in zip(streams, (self.full, self.afull)):
            sizes += [inf.P * full, inf.P] if self.counts else [inf.P * full]
        sizes += [math.prod(f.rows_shape(inf)) for inf, f in streams if f is not None]
        ends = list(itertools.accumulate(sizes))
        return tuple(zip([0] + ends, ends))

    def pack(self, idx, nb_sent, codes=None, na_sent=None):
        """Device: idx [nb, G, n] and, with audio packets, the audio codes [G, >= na, n], with ``counts`` each stream's counts
        uint8 [G, P] (else None) -> the rows uint8 [G, bytes of layout(n)] for ONE read-back: ops.idx_pack_packets per stream,
        then ops.fec_parity per stream with a Fec -- pack tactile, pack audio, tactile parity, audio parity, the order inside the
        captured steady step -- then one cat.  A row of a single part is the packed bodies themselves, a view: no copy kernel."""
        import torch
        from . import ops
        G, n = idx.shape[1:]
        streams, parts = self._streams(n), []
        data = [(idx, 0)] + ([] if self.audio is None else [(codes[:, :self.audio[1]], 1)])                # indices, their book_dim
        sent = [nb_sent, na_sent] if self.counts else [None, None]
        bodies = [ops.idx_pack_packets(x, inf.K, self.packet_tok, book_dim=d) for (inf, _), (x, d) in zip(streams, data)]
        for b, c in zip(bodies, sent):
            parts += [b.reshape(G, -1)] if c is None else [b.reshape(G, -1), c]
        parts += [ops.fec_parity(b, c, inf, f).reshape(G, -1) for (inf, f), b, c in zip(streams, bodies, sent) if f is not None]
        return parts[0] if len(parts) == 1 else torch.cat(parts, dim=1)

    def frame_item(self, row, n, seq_base=0):
        """Host: ONE item's row of ``pack``'s array -> the headers, data packets numbered from ``seq_base`` (packets.frame) and a
        stream's parity packets from seq_base // fec.group (packets.frame_fec): (tactile_packets,) or (tactile_packets,
        audio_packets), then -- only when some Fec is set -- one parity list per stream that may have one: (fec_packets,), with
        audio packets (fec_packets, audio_fec_packets), [] for a stream without a Fec."""
        import numpy as np
        from .packets import frame, frame_fec
        row, spans, streams = np.asarray(row, np.uint8).reshape(-1), self.layout(n), self._streams(n)
        if row.size != spans[-1][1]:
            raise ValueError(f"_TxBack.frame_item: a row of {row.size} bytes for {spans[-1][1]} of {n} tokens")
        part = iter([row[a:b] for a, b in spans])                            # consumed in layout order: data parts, then parity parts
        out = ()
        for inf, _ in streams:
            body = next(part)
            out += (frame(body, inf, nb_sent=next(part) if self.counts else None, seq_base=seq_base),)
        if self.fec is None and self.audio_fec is None:
            return out
        return out + tuple([] if f is None else frame_fec(next(part), inf, f, seq_base=seq_base // int(f.group)) for inf, f in streams)


class SenderStep(NamedTuple):
    """What one ``push`` / ``finish`` of a sender session does: ``emit`` -- whether an encoder window runs; then the window's ``w``
    samples, the ``drop`` samples the buffer loses, the tokens [lo, hi) of the window that are emitted (``finish`` without an
    emit: hi = the tokens the samples in hand make, for its StreamInfo); and the session afterwards: ``fill`` samples held,
    ``start`` the token buf[0] belongs to, ``chunk`` the next chunk to emit."""
    emit: bool
    w: int
    drop: int
    lo: int
    hi: int
    fill: int
    start: int
    chunk: int


def sender_step(fill: int, start: int, chunk: int, n: int, last: bool = False) -> SenderStep:
    """The host arithmetic of a sender session (StreamSender and StreamSenderPool both call it; ``sender_schedule`` says the same
    in tokens): the step that takes ``n`` new samples with ``fill`` samples held from token ``start`` on and ``chunk`` the next
    chunk to emit.  A push (n = 320*m, 1 <= m <= 16) emits chunk c once 16c + 16 + 8 tokens are in hand: the window is every
    sample from ``start`` up to that token, and the samples before token 16c + 16 - 8 are dropped.  ``finish`` (``last``, any n)
    encodes all fill + n samples once and keeps nothing; it emits unless no token lies past ``lo`` (an item shorter than a token)."""
    fill, start, c, n, last = int(fill), int(start), int(chunk), int(n), bool(last)
    if fill < 0 or start < 0 or c < 0 or n < 0 or fill % HOP and not last:
        raise ValueError(f"sender_step: fill = {fill}, start = {start}, chunk = {c}, n = {n}")
    lo = CHUNK_TOK * c - start
    if last:
        T_w = enc_tokens(fill + n)
        if T_w <= lo:
            return SenderStep(False, 0, 0, lo, T_w, 0, start, c)
        return SenderStep(True, fill + n, fill + n, lo, T_w, 0, start, (start + T_w + CHUNK_TOK - 1) // CHUNK_TOK)
    if n % HOP or not HOP <= n <= PUSH_MAX_TOK * HOP:
        raise ValueError(f"sender_step: a push of {n} samples")
    end = CHUNK_TOK * (c + 1) + ENC_HALO_TOK                              # the first token the window of chunk c does not need
    if start + (fill + n) // HOP < end:
        return SenderStep(False, 0, 0, 0, 0, fill + n, start, c)
    new_start = CHUNK_TOK * (c + 1) - ENC_HALO_TOK
    drop = HOP * (new_start - start)
    return SenderStep(True, HOP * (end - start), drop, lo, lo + CHUNK_TOK, fill + n - drop, new_start, c + 1)


def sender_step_stateful(fill: int, start: int, chunk: int, n: int, last: bool = False) -> SenderStep:
    """``sender_step`` for encoder="stateful" (StreamSender and StreamSenderPool both call it).  The schedule
    is sender_schedule's -- chunk c leaves with the push after which 16c + 24 tokens are in hand -- but the encoders are fed only
    the samples they have not seen: the buffer holds ``fill`` un-encoded samples from token ``start`` on (``start`` tokens are
    encoded: samples_before = 320*start).  An emitting push feeds the w samples up to token 16c + 24 -- 24 tokens for chunk 0, 16
    in the steady state -- and the buffer drops exactly those (drop = w); ``finish`` feeds everything left (any count, none too:
    the stage tails alone are flushed against the true edge).  [lo, hi) are the emitted tokens relative to token ``start``, as in
    sender_step; here the tokens of chunk c lie up to 8 tokens BEFORE the samples fed, so lo may be negative: the stateful encode
    returns exactly hi - lo tokens and nothing is sliced."""
    fill, start, c, n, last = int(fill), int(start), int(chunk), int(n), bool(last)
    if fill < 0 or start < 0 or c < 0 or n < 0 or fill % HOP and not last:
        raise ValueError(f"sender_step_stateful: fill = {fill}, start = {start}, chunk = {c}, n = {n}")
    lo = CHUNK_TOK * c - start
    if last:
        T = enc_tokens(HOP * start + fill + n)                            # the item's tokens
        if T <= CHUNK_TOK * c:
            return SenderStep(False, 0, 0, lo, T - start, 0, start, c)
        return SenderStep(True, fill + n, fill + n, lo, T - start, 0, start, (T + CHUNK_TOK - 1) // CHUNK_TOK)
    if n % HOP or not HOP <= n <= PUSH_MAX_TOK * HOP:
        raise ValueError(f"sender_step_stateful: a push of {n} samples")
    end = CHUNK_TOK * (c + 1) + ENC_HALO_TOK                              # the first token chunk c does not need
    if start + (fill + n) // HOP < end:
        return SenderStep(False, 0, 0, 0, 0, fill + n, start, c)
    w = HOP * (end - start)
    return SenderStep(True, w, w, lo, lo + CHUNK_TOK, fill + n - w, end, c + 1)


class SenderGroup(NamedTuple):
    """Sender sessions of one tick that share a launch sequence: ``key`` = ("append",), ("emit", min(chunk, 1)) or
    ("finish", fill + n, lo); ``sids`` ascending; ``w`` the window in samples and [lo, hi) the tokens of it that are emitted
    (all zero for the append group); ``steps`` the SenderStep of every member, in the order of ``sids``."""
    key: tuple
    sids: Tuple[int, ...]
    w: int
    lo: int
    hi: int
    steps: Tuple[SenderStep, ...]


def sender_pool_groups(sessions, stateful: bool = False) -> List[SenderGroup]:
    """``sessions``: (sid, fill, start, chunk, n, last) of every session that takes a step this tick (``sender_step``'s
    arguments).  -> the groups that do device work, ordered by key.

    Sessions may share a launch sequence only when their launch parameters agree.  The sample-state kernel takes fill, n and drop
    per session, so what must agree is what the encoders and everything after them see: the window length and the emitted tokens.
      * pushes that emit nothing need the sample-state launch alone: ONE group, ("append",), w = 0;
      * a push that emits chunk 0 runs the 24-token window with lo = 0, one that emits any later chunk the 32-token window with
        lo = 8, whatever it holds and whatever it pushed: ("emit", 0) and ("emit", 1);
      * a finisher's window is all it holds, fill + n samples, emitted from lo on: ("finish", fill + n, lo).  One whose window
        holds no token past lo does no device work and is in no group.
    Nothing coarser is sound: windows of different lengths are never merged by padding, only a true edge is exact.

    ``stateful`` (encoder="stateful", ``sender_step_stateful``): the same keys, read as what the encoder STAGE plan depends on.
    encoder_stage_plan depends on samples_before = 320*start only through chunk 0 (nothing encoded) against any later chunk
    (16c + 8 tokens encoded: every stage's tail is full and its column count mod its stride is that of every later chunk), so
    ("emit", min(chunk, 1)) stands; a finisher's plan depends on that class and on its un-encoded sample count:
    ("finish", fill + n, min(chunk, 1))."""
    seen, by_key, step_of = set(), {}, {}
    for sid, fill, start, chunk, n, last in sessions:
        if sid in seen:
            raise ValueError(f"sender_pool_groups: session {sid} is listed twice")
        seen.add(sid)
        st = (sender_step_stateful if stateful else sender_step)(fill, start, chunk, n, last)
        if last:
            if not st.emit:
                continue
            key = ("finish", st.w, min(int(chunk), 1) if stateful else st.lo)
        else:
            key = ("emit", min(int(chunk), 1)) if st.emit else ("append",)
        by_key.setdefault(key, []).append(sid)
        step_of[sid] = st
    out = []
    for key in sorted(by_key):
        sids = tuple(sorted(by_key[key]))
        first = step_of[sids[0]]
        assert all((step_of[s].w, step_of[s].lo, step_of[s].hi) == (first.w, first.lo, first.hi) for s in sids)
        out.append(SenderGroup(key, sids, first.w, first.lo, first.hi, tuple(step_of[s] for s in sids)))
    return out


def _f32_only(who):
    """The sessions that claim an equality chunk by chunk refuse the opt-in arithmetic modes: they scale per item, so a window
    changes their arithmetic."""
    from . import ops
    if ops.get_arith() != "f32":
        raise ValueError(f"{who}: arithmetic mode {ops.get_arith()!r} scales per item; only 'f32' is equal chunk by chunk")


def _capture(dev, state, step):
    """A session's steady step as a graph -> (CUDAGraph, what ``step()`` returned inside the capture).  ``step`` runs once
    eagerly first, at the steady shape, so that nothing is built during the capture; it moves the session on, so the ``state``
    tensors are saved before and restored after it."""
    import torch
    keep = [t.clone() for t in state]
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
        for t, k in zip(state, keep):
            t.copy_(k)
        with torch.cuda.graph(g, stream=s):
            out = step()
    torch.cuda.current_stream().wait_stream(s)
    return g, out


class _SessionTable:
    """The session bookkeeping of a pool, receiver and sender alike: ``slots`` row blocks of the state buffers, the free ones
    ascending, and per open session ``_sess[sid]`` = [slot, ...the kind's host state]; a sid is never reused."""

    def _init_sessions(self, slots):
        self.slots = slots
        self._free = list(range(slots))                                                # ascending: open() takes the lowest
        self._sess = {}
        self._next_sid = 0

    @property
    def active(self):
        """The sids of the open sessions, ascending."""
        return tuple(sorted(self._sess))

    @property
    def free(self):
        """Slots no session holds."""
        return len(self._free)

    def _get(self, sid, what):
        from ._lib import MvqError
        try:
            return self._sess[sid]
        except (KeyError, TypeError):
            raise MvqError(f"{self._who}: {what}: no open session {sid!r} (never opened, finished or closed)") from None

    def _take_slot(self):
        """The lowest free slot, for ``open`` to reset and hand to ``_new_session``."""
        from ._lib import MvqError
        if not self._free:
            raise MvqError(f"{self._who}: all {self.slots} slots hold a session")
        return self._free.pop(0)

    def _new_session(self, slot, *state):
        sid, self._next_sid = self._next_sid, self._next_sid + 1
        self._sess[sid] = [slot, *state]
        return sid

    def close(self, sid):
        """Abandon session ``sid`` without flushing it; its slot is free again."""
        import bisect
        slot = self._get(sid, "close")[0]
        del self._sess[sid]
        bisect.insort(self._free, slot)


def _sender_samples(who, what, a, t, B, fill, tail=False):
    """The checks of a sender's samples, before any launch -> (a, t, n): ``a`` / ``t`` float tensors [B, 1, n] of one length; a
    push carries 320*m samples, 1 <= m <= 16, ``finish`` (``tail``) any count."""
    import torch
    a, t = torch.as_tensor(a), torch.as_tensor(t)
    for x, name in ((a, "a"), (t, "t")):
        if x.dim() != 3 or x.shape[1] != 1 or not x.dtype.is_floating_point:
            raise ValueError(f"{who}.{what}: {name} must be a float tensor [B, 1, samples], got {tuple(x.shape)}")
    if a.shape[0] != B or t.shape[0] != B:
        raise ValueError(f"{who}.{what}: samples of {a.shape[0]} / {t.shape[0]} items for a session of batch {B}")
    if a.shape[2] != t.shape[2]:
        raise ValueError(f"{who}.{what}: {a.shape[2]} audio and {t.shape[2]} tactile samples; the two modalities advance together")
    n = int(a.shape[2])
    if not tail and (n % HOP or not HOP <= n <= PUSH_MAX_TOK * HOP):
        raise ValueError(f"{who}.push: {n} samples; a push is {HOP}*m samples, 1 <= m <= {PUSH_MAX_TOK} "
                         "(anything else goes to finish)")
    if tail and fill + n > (1 << 24):
        raise ValueError(f"{who}.finish: {n} samples")
    return a, t, n


class _SenderCore:
    """What StreamSender and StreamSenderPool share: the configuration, the state buffers -- per session two rows of ``buf``
    (audio, tactile; 48*320 samples each) and a row of ``carry`` [sessions, C] -- and THE device sequence from an encoder window
    to packet bodies, written once.  With ``sl`` None it works on every session of the buffers (the lockstep sender); with ``sl``
    = (slots, slots_dev), the host list of a group's slots and its int32 device copy, on those sessions of a pool: the carried
    tokens go through a dense [G, C] copy (ops.stream_rows), everything else is the same launches on the group's window."""

    def __init__(self, who, net, packet_tok, books_use, sessions, buf_shape, rate=None, audio="codes", audio_books=None,
                 audio_rate=None, fec=None, audio_fec=None, encoder="window"):
        import torch
        from . import proposed
        from .packets import StreamInfo, _check
        if packet_tok < 1 or CHUNK_TOK % packet_tok:
            raise ValueError(f"{who}: packet_tok = {packet_tok} does not divide the {CHUNK_TOK}-token chunk "
                             "(a packet must never straddle two chunks)")
        if sessions < 1:
            raise ValueError(f"{who}: {'batch' if who == 'StreamSender' else 'slots'} must be at least 1")
        if encoder not in ("window", "stateful"):
            raise ValueError(f"{who}: encoder must be 'window' or 'stateful', not {encoder!r}")
        self.encoder = encoder
        _f32_only(who if encoder == "window" else f"{who}(encoder='stateful')")
        assert proposed.AR_CHUNK_TOK == CHUNK_TOK
        for enc in (net.A_ENC, net.T_ENC):
            if tuple(enc._desc[1]) != ENC_RATES:
                raise ValueError(f"{who}: encoder strides {tuple(enc._desc[1])}; the window schedule is measured for {ENC_RATES}")
        self.K = int(net.vq.n_embed)
        self.nb = int(net.vq.n_books) if books_use is None else max(0, min(int(books_use), int(net.vq.n_books)))
        _check(StreamInfo(self.K, self.nb, CHUNK_TOK, packet_tok))
        self.net, self.packet_tok, self.books_use = net, packet_tok, books_use
        if audio not in ("codes", "packets"):
            raise ValueError(f"{who}: audio must be 'codes' or 'packets', not {audio!r}")
        if audio == "codes" and (audio_books is not None or audio_rate is not None):
            raise ValueError(f"{who}: audio_books / audio_rate go with audio='packets'")
        self.audio_packets = audio == "packets"
        self.audio_rate = self.na = None
        if self.audio_packets:                                                         # both loops run closed (proposed.encode_latents_with_indices)
            from .packets import Rate
            self.audio_rate, self.na, _ = net._audio_rate_resolve(audio_rate, audio_books, packet_tok)
            self.K_audio = int(net.A_QUANT.codebook_size)
            rate = Rate() if rate is None else rate
        if rate is not None:
            net._rate_resolve(rate, books_use, packet_tok)                             # ValueError before any session state exists
        self.rate = rate
        if audio_fec is not None and not self.audio_packets:
            raise ValueError(f"{who}: audio_fec goes with audio='packets'")
        if fec is not None:                                                            # ValueError before any session state exists
            net._fec_resolve(fec, self.K, self.nb, packet_tok)
        if audio_fec is not None:
            net._fec_resolve(audio_fec, self.K_audio, self.na, packet_tok, what="audio_fec")
        self.fec, self.audio_fec = fec, audio_fec
        self._back = _TxBack(self.K, self.nb, packet_tok, (self.K_audio, self.na) if self.audio_packets else None, rate is not None,
                             fec, audio_fec)
        self.dev = net.proj_up.weight.device
        self.C = net.proj_up.out_channels
        self.n_audio_books = net.A_QUANT.n_codebooks
        self.buf = torch.zeros(*buf_shape, device=self.dev)                            # per session: an audio and a tactile row
        self.carry = torch.zeros(sessions, self.C, device=self.dev)                    # per session: z_run[..., -1] of the chunk before
        self.enc_state = None                                                          # stateful: (audio, tactile) stage tails [sessions, S]
        if encoder == "stateful":                                                      # allocated once, never cleared: a new session reads no tail
            self.enc_state = (net.A_ENC.stream_state(sessions), net.T_ENC.stream_state(sessions))
        self._step = sender_step if encoder == "window" else sender_step_stateful

    def _branches_stateful(self, a_w, t_w, n_tok, before, last, sl=None):
        """``_branches`` for encoder="stateful": the same two stack calls under the same rule, each A_ENC / T_ENC.forward_stream on
        the samples that were not encoded yet (``before`` samples were; enc_state moves on in place).  They return exactly the
        chunk's n_tok tokens, so nothing is sliced."""
        net = self.net
        slots, slots_dev = (None, None) if sl is None else sl
        sa, st_ = self.enc_state

        def audio():
            za = net.A_ENC.forward_stream(sa, a_w, before, last, slots=slots, slots_dev=slots_dev)
            qa, codes, *_ = net.A_QUANT(za)
            return za, qa, codes
        (za, qa, codes), zt = net._two_streams(a_w, audio, lambda: net.T_ENC.forward_stream(st_, t_w, before, last, slots=slots,
                                                                                            slots_dev=slots_dev))
        assert za.shape[-1] == zt.shape[-1] == n_tok
        return qa, codes, zt, za

    def _branches(self, a_w, t_w, lo, hi):
        """The two encoders on the window and the audio quantiser on tokens [lo, hi) of it -> (qa, codes, zt, the encoder output
        the quantiser searched); one or two HIP streams as ``ProposedEval._two_streams`` decides."""
        net = self.net

        def audio():
            za = net.A_ENC(a_w)
            za_c = za[..., lo:hi].contiguous()
            qa, codes, *_ = net.A_QUANT(za_c)
            return za, za_c, qa, codes
        (_, za_c, qa, codes), zt = net._two_streams(a_w, audio, lambda: net.T_ENC(t_w)[..., lo:hi].contiguous())
        return qa, codes, zt, za_c

    def _encode(self, win, lo, hi, sl=None, before=None, last=False):
        """Device: the window win[2, G, w] (audio rows, then tactile rows) -> latents of tokens [lo, hi) of it -> (the rows uint8
        [G, bytes] of ``_TxBack.pack`` for one read-back, audio codes int64 [G, 32, hi - lo]); the carried token moves on in place.
        With ``self.rate`` the loop runs closed (on the books each packet carries and on qa from the codes, as the receiver will),
        with audio packets on both streams; the counts and, with ``self.fec`` / ``self.audio_fec``, the parity rows of the window's
        packets (the window starts on a chunk, so its groups are the item's) ride in the same rows.
        encoder="stateful": ``win`` holds only the samples not encoded yet, ``before`` samples were (``last``: the finish), and the
        latents come from ``_branches_stateful``; everything behind them is the same."""
        from . import ops
        a_w, t_w = win[0].unsqueeze(1), win[1].unsqueeze(1)
        if self.enc_state is None:
            qa, codes, zt, za = self._branches(a_w, t_w, lo, hi)
        else:
            qa, codes, zt, za = self._branches_stateful(a_w, t_w, hi - lo, before, last, sl)
        carry = self.carry if sl is None else ops.stream_rows(self.carry, sl[0], slots_dev=sl[1])
        nb_sent = na_sent = None
        if self.audio_packets:                                                         # qa of the stages each audio packet carries
            qa, _, na_sent = self.net.A_QUANT.rate(za, codes, self.audio_rate, self.packet_tok, self.na)
        elif self.rate is not None:                                                    # qa from the codes, as the receiver forms it
            qa = self.net.A_QUANT.from_codes(codes)[0]
        del za                                                                         # recorded on two streams: freed no later than it was
        if self.rate is not None:
            _, _, idx, _, nb_sent = self.net._ar_latents(qa, zt, self.books_use, z_prev=carry, z_last_out=carry, rate=self.rate,
                                                         packet_tok=self.packet_tok)
        else:
            _, _, idx = self.net._ar_latents(qa, zt, self.books_use, want_indices=True, z_prev=carry, z_last_out=carry)
        # A session that ends needs no carry: ``close`` frees its slot, and StreamSenderPool.open zeroes carry[slot] before anyone
        # reads it again.
        if sl is not None and not last:
            ops.stream_rows(self.carry, sl[0], rows=carry, slots_dev=sl[1])
        return self._back.pack(idx, nb_sent, codes, na_sent), codes

    # ---------------------------------------------------------------------------------------------------------- what a call returns
    def _frame_one(self, row, n_tok, chunk):
        """Host: ONE session's row of the read-back, the session being at chunk ``chunk`` -> ``_TxBack.frame_item``'s values."""
        return self._back.frame_item(row, n_tok, chunk * CHUNK_TOK // self.packet_tok)

    def _frame(self, row, n_tok, chunk, codes):
        """Host: ONE session's row of the read-back -> what its push returns, the session being at chunk ``chunk``."""
        return self._with_codes(self._frame_one(row, n_tok, chunk), codes)

    def _with_codes(self, framed, codes):
        """``_TxBack.frame_item``'s values (of one item, or per-item lists of them) -> a push's: without audio packets the audio
        codes sit behind the tactile packets."""
        return framed if self.audio_packets else (framed[0], codes) + framed[1:]

    def _nothing(self, items=1):
        """What a push of ONE session that completes no chunk returns: a real result's length, every list empty, the codes
        [items, 32, 0]."""
        import torch
        if self.audio_packets:
            return ([], []) + (([], []) if self.fec is not None or self.audio_fec is not None else ())
        return ([], torch.empty(items, self.n_audio_books, 0, dtype=torch.int64, device=self.dev)) + (([],) if self.fec is not None else ())

    def _infos(self, T):
        from .packets import StreamInfo
        info = (StreamInfo(self.K, self.nb, T, self.packet_tok),)
        return info + (StreamInfo(self.K_audio, self.na, T, self.packet_tok),) if self.audio_packets else info

    def _finished(self, out, T):
        """finish's return value: the two data elements, the StreamInfo(s), then the parity lists (sessions with a Fec)."""
        return tuple(out[:2]) + self._infos(T) + tuple(out[2:])


class StreamSender(_SenderCore):
    """A sender session for ``batch`` items advancing in lockstep: ``push`` the next samples of both modalities (320*m each,
    1 <= m <= 16), get back the tactile packets and audio codes of the 16-token chunk they complete (nothing when they complete
    none); ``finish`` takes the remaining samples (any count, none too) and flushes.

    Per item the packets of all pushes and ``finish`` concatenated equal ``compress_packets``' packets byte for byte, the audio
    codes concatenated equal the whole-item codes, and ``finish`` returns the same ``StreamInfo`` -- for ``ops.get_arith() ==
    "f32"`` (the opt-in arithmetic modes scale per item, so a window changes their arithmetic; they are refused) and for
    modalities of one length.  Chunk c leaves once 8 tokens past its end are in hand: the algorithmic latency is one chunk plus
    the encoder look-ahead, 213.3 + 106.7 ms, instead of the whole item.

    An emitting ``push`` runs, in order: ops.stream_samples (the sample buffer [2B, 48*320]: window out, buffer moved on, one
    launch for both modalities) -> A_ENC and T_ENC on the window (``sender_schedule``; one or two HIP streams as
    ``ProposedEval._two_streams`` decides) -> the chunk's 16 exact tokens -> A_QUANT -> _ar_latents(want_indices=True, z_prev=carry,
    z_last_out=carry) -> _TxBack.pack -> ONE device-to-host copy of the rows -> _TxBack.frame_item(seq_base=).  A push that
    emits nothing is the append launch alone.  All session state is in fixed device buffers (samples [2B, 15360], carry [B, C]).

    ``graph=True``: the steady step (a push of exactly 16 tokens that completes a chunk after the first: the 32-token window) is
    captured once as a graph, at the buffer fill it first occurs with, and replayed after the host has written the samples into
    the static input buffer whenever a push has that shape again -- with 16-token pushes the fill before every push is the same
    (16 tokens when the first push was 8, 24 when every push was 16).  Everything else runs eagerly.

    ``rate`` (packets.Rate): closed-loop sender rate control, the session's output then equals compress_packets(rate=).  The book
    count of each packet is decided on the device and comes back behind the bodies in the push's one read-back; it never reaches
    the host before that, so the captured steady step replays with other decisions.

    ``audio="packets"`` (with ``audio_books`` / ``audio_rate``, as compress_packets_av takes them): the audio codes leave in layered
    packets too.  ``push`` then returns (tactile_packets, audio_packets), both with the stream's sequence numbers, and ``finish``
    (tactile_packets, audio_packets, StreamInfo, audio StreamInfo); per item their concatenation equals compress_packets_av byte
    for byte.  Both loops run closed (``rate`` None is Rate()); both streams' bodies and counts come back in the push's ONE
    read-back, so ``graph=True`` keeps working.  The default ``audio="codes"`` is the behaviour above exactly.

    ``fec`` / ``audio_fec`` (packets.Fec; ``audio_fec`` needs ``audio="packets"``; both None: the behaviour above exactly): forward
    error correction, DESIGN.md section 20.  The parity launch sits behind the packing inside the device step -- so inside the
    captured steady step -- and the parity rows ride behind everything else in the push's ONE read-back.  Every ``push`` then
    returns its usual values and then the chunk's parity packets: (tactile_packets, audio_codes, fec_packets), or with audio
    packets (tactile_packets, audio_packets, fec_packets, audio_fec_packets) where a stream without a Fec gets empty lists;
    ``finish`` returns its usual values and then the same parity lists.  Groups are numbered across the stream: chunk c's start at
    c * (16 // packet_tok // group).  Per item the concatenation equals compress_packets(fec=) / compress_packets_av(fec=,
    audio_fec=) byte for byte, data and parity.  A Fec with parity = r > 1 emits r packets per group (``MF``, then ``MR``).

    ``encoder="stateful"`` (the default "window" is the sequence above, launch for launch): instead of A_ENC and
    T_ENC on the 24- / 32-token window, A_ENC / T_ENC.forward_stream on the samples that were not encoded yet (24 tokens for chunk 0,
    then 16; ``sender_step_stateful``) -- every encoder stage keeps the tail of its own input in enc_state (two [B, S] buffers) and
    returns exactly the chunk's tokens; the sample buffer holds un-encoded samples only.  Every push / finish returns exactly the
    window mode's values; the steady step stays ONE captured graph; everything behind the latents is untouched."""

    def __init__(self, net, packet_tok=2, batch=1, books_use=None, graph=False, rate=None, audio="codes", audio_books=None,
                 audio_rate=None, fec=None, audio_fec=None, encoder="window"):
        packet_tok, batch = int(packet_tok), int(batch)
        super().__init__("StreamSender", net, packet_tok, books_use, batch, (2 * batch, SEND_CAP_TOK * HOP), rate=rate, audio=audio,
                         audio_books=audio_books, audio_rate=audio_rate, fec=fec, audio_fec=audio_fec,   # buffer: audio rows, then tactile rows
                         encoder=encoder)
        self.batch, self.graph = batch, bool(graph)
        self.fill = 0                                                                  # valid samples of every buffer row
        self.start = 0                                                                 # the token buf[:, 0] belongs to
        self.chunk = 0                                                                 # the next chunk to emit
        self.finished = False
        self._g = None                                                                 # (graph, fill, x_static, bodies_static, codes_static)

    @property
    def tokens(self):
        """Tokens of samples received so far."""
        return self.start + self.fill // HOP

    # ------------------------------------------------------------------------------------------------------------ stages
    def _device_step(self, x, fill, w, drop, lo, hi, before=None, last=False):
        """Device: samples -> window -> latents of tokens [lo, hi) of the window -> (_encode's rows uint8 [B, bytes], audio codes
        int64 [B, 32, hi - lo]); the buffer and the carried token move on in place (encoder="stateful": the encoder states too,
        ``before`` = the samples encoded so far)."""
        from . import ops
        return self._encode(ops.stream_samples(self.buf, fill, x, w, drop).view(2, self.batch, w), lo, hi, before=before, last=last)

    def _samples(self, a, t, what, tail=False):
        """The checks of a push, before any launch -> (a, t) and n."""
        return _sender_samples("StreamSender", what, a, t, self.batch, self.fill, tail)

    def _upload(self, a, t, n):
        import torch
        x = torch.empty(2 * self.batch, n, device=self.dev)
        x[:self.batch].copy_(a.reshape(self.batch, n))
        x[self.batch:].copy_(t.reshape(self.batch, n))
        return x

    def _framed(self, bodies, codes, n_tok):
        """ONE device-to-host copy of the rows, then the headers with the stream's sequence numbers (_frame_one per item, every
        item at the session's chunk), each value a list per item."""
        items = [self._frame_one(row, n_tok, self.chunk) for row in bodies.cpu().numpy().reshape(self.batch, -1)]
        return self._with_codes(tuple(list(c) for c in zip(*items)), codes)

    def _nothing(self):
        return tuple([[] for _ in range(self.batch)] if isinstance(v, list) else v for v in super()._nothing(self.batch))

    def _open(self, what):
        from ._lib import MvqError
        if self.finished:
            raise MvqError(f"StreamSender: {what} after finish")
        _f32_only("StreamSender")

    # ------------------------------------------------------------------------------------------------------------ session
    def push(self, a, t):
        """``a`` / ``t`` [B, 1, 320*m], 1 <= m <= 16: the next samples of the audio and the tactile signal ->
        (tactile_packets, audio_codes): B lists of framed packets (``bytes``) with the stream's sequence numbers
        16c/packet_tok ... and int64 [B, 32, 16] on the device when the push completes chunk c; B empty lists and [B, 32, 0]
        when it completes none."""
        import torch
        from . import ops
        self._open("push")
        a, t, n = self._samples(a, t, "push")
        st = self._step(self.fill, self.start, self.chunk, n)
        with torch.no_grad():
            if not st.emit:
                ops.stream_samples(self.buf, self.fill, self._upload(a, t, n), 0, 0)
                self.fill = st.fill
                return self._nothing()
            plan = (self.fill, st.w, st.drop, st.lo, st.hi) + (() if self.enc_state is None else (HOP * self.start,))
            if self.graph and self.chunk > 0 and n == CHUNK_TOK * HOP and (self._g is None or self._g[1] == self.fill):   # the steady step
                bodies, codes = self._replay(a, t, n, plan)
            else:
                bodies, codes = self._device_step(self._upload(a, t, n), *plan)
            out = self._framed(bodies, codes, CHUNK_TOK)
            self.fill, self.start, self.chunk = st.fill, st.start, st.chunk
            return out

    def finish(self, a=None, t=None):
        """Flush: optionally the remaining samples ``a`` / ``t`` [B, 1, n] (any n, no multiple of 320 needed), then every
        remaining chunk from ONE encoder window that ends at the item's true end, the token carried from chunk to chunk
        -> (tactile_packets, audio_codes, StreamInfo(K, nb, T, packet_tok)).  Runs eagerly.  The session accepts nothing afterwards."""
        import torch
        from .packets import StreamInfo
        self._open("finish")
        if (a is None) != (t is None):
            raise ValueError("StreamSender.finish: the remaining samples of both modalities, or of neither")
        n = 0
        if a is not None:
            a, t, n = self._samples(a, t, "finish", tail=True)
        st = self._step(self.fill, self.start, self.chunk, n, last=True)
        if st.w > ENC_STREAM_MAX_N and self.enc_state is not None:
            raise ValueError(f"StreamSender.finish: {st.w} samples left to encode; encoder='stateful' takes at most {ENC_STREAM_MAX_N} in one step")
        with torch.no_grad():
            if not st.emit:                                              # an item shorter than one token: nothing to send
                self.finished = True
                return self._finished(self._nothing(), self.start + max(st.hi, 0))
            x = self._upload(a, t, n) if n else torch.empty(2 * self.batch, 0, device=self.dev)
            if self.enc_state is None:
                bodies, codes = self._device_step(x, self.fill, st.w, st.drop, st.lo, st.hi)
            else:
                bodies, codes = self._device_step(x, self.fill, st.w, st.drop, st.lo, st.hi, HOP * self.start, True)
            out = self._framed(bodies, codes, st.hi - st.lo)
            self.fill, self.chunk, self.finished = st.fill, st.chunk, True
            return self._finished(out, self.start + st.hi)

    def _replay(self, a, t, n, plan):
        """The steady step as a graph: captured at its first use (after one eager run at that shape on copies of the state, so
        that nothing is built during the capture), then replayed with the samples written into the static input buffer.  The
        audio codes come back as a copy: the graph's own output buffer is overwritten by the next replay."""
        B = self.batch
        if self._g is None:
            x_s = self._upload(a, t, n)
            state = (self.buf, self.carry) + (() if self.enc_state is None else self.enc_state)
            g, (bodies_s, codes_s) = _capture(self.dev, state, lambda: self._device_step(x_s, *plan))
            self._g = (g, plan[0], x_s, bodies_s, codes_s)
        else:
            g, _, x_s, bodies_s, codes_s = self._g
            x_s[:B].copy_(a.reshape(B, n))
            x_s[B:].copy_(t.reshape(B, n))
        g.replay()
        return bodies_s, codes_s.clone()


class StreamSenderNative:
    """``StreamSender`` fed at the sensors' own rates: ``in_rates`` = (audio Hz, tactile Hz), by default the
    reference's 44.1 kHz microphone and 3 kHz accelerometer.  It is two ``resample.StreamResampleRational`` (-> 24 kHz) in front of
    one inner ``StreamSender(net, **sender_options)``; each resampler lags by the filter blocks of exactly one 320-sample token
    (``native_token_plan``: 4 blocks of 147 samples for 44.1 kHz, 40 of 1 for 3 kHz), so every call hands the inner session whole
    tokens.  That lag is the algorithmic latency this front end adds: one token-time, 13.3 ms, on top of the inner session's
    213.3 + 106.7 ms.

    ``push(a, t)``: ``a`` [B, 1, tok_a*m], ``t`` [B, 1, tok_t*m] with one m, 1 <= m <= 16 (``samples_per_token`` = (tok_a, tok_t):
    (588, 40) for the default rates) -> two resample launches, then the inner ``push`` of the 320*k samples they completed, whose
    return value is returned unchanged: k = m - 1 for the first push (one token completes none: the inner session's "nothing"),
    k = m afterwards.  ``finish(a=None, t=None)`` takes the remaining native samples (any count, per modality, or none), flushes both
    resamplers, crops the two 24 kHz tails to the shorter (the reference's crop_match), feeds whole tokens through inner pushes of at
    most 16 and the remainder to the inner ``finish``, and returns ``finish``'s tuple with what those pushes returned in front, per item.

    Per item, all pushes and ``finish`` concatenated equal compress_packets(*crop_match(Resample(sr_a, 24000)(a), Resample(sr_t,
    24000)(t)), ...) with the same options (compress_packets_av for audio="packets"): packets and parity byte for byte, equal
    StreamInfos, equal audio codes.  Refused with ValueError before anything is allocated: rates at which a token is no whole number
    of filter blocks (2800 Hz) or the resampler state would exceed 1024 samples, a rate that already is 24 kHz, and whatever the
    inner StreamSender refuses.  ``graph=True`` passes through: the inner steady step stays its one captured graph, the two resample
    launches run eagerly in front of it."""

    def __init__(self, net, in_rates=(44100, 3000), **sender_options):
        from .resample import StreamResampleRational
        try:
            ra, rt = (int(r) for r in in_rates)
        except (TypeError, ValueError):
            raise ValueError(f"StreamSenderNative: in_rates must be (audio Hz, tactile Hz), not {in_rates!r}") from None
        for r in (ra, rt):
            if r <= 0 or r == LINK_SR:
                raise ValueError(f"StreamSenderNative: an input rate of {r} Hz (positive, and not the link's own {LINK_SR} Hz: "
                                 "StreamSender takes those samples as they are)")
        plans = tuple(native_token_plan(r, LINK_SR) for r in (ra, rt))                 # ValueError before any allocation
        self.in_rates = (ra, rt)
        self.samples_per_token = (plans[0][4], plans[1][4])
        self.inner = StreamSender(net, **sender_options)
        self.batch, self.dev = self.inner.batch, self.inner.dev
        self.rs = tuple(StreamResampleRational(r, LINK_SR, self.batch, device=self.dev, hold=p[3]) for r, p in zip((ra, rt), plans))

    @property
    def tokens(self):
        """Tokens of 24 kHz samples handed to the inner session so far."""
        return self.inner.tokens

    @property
    def finished(self):
        return self.inner.finished

    def _native(self, x, name, what):
        import torch
        x = torch.as_tensor(x)
        if x.dim() != 3 or x.shape[0] != self.batch or x.shape[1] != 1 or not x.dtype.is_floating_point:
            raise ValueError(f"StreamSenderNative.{what}: {name} must be a float tensor [B={self.batch}, 1, samples], got {tuple(x.shape)}")
        return x

    def push(self, a, t):
        """The next ``m`` tokens of native samples of both modalities (class docstring) -> the inner ``StreamSender.push``'s value."""
        import torch
        self.inner._open("push")
        a, t = self._native(a, "a", "push"), self._native(t, "t", "push")
        (ta, tt), (na, nt) = self.samples_per_token, (a.shape[2], t.shape[2])
        m = na // ta
        if na != ta * m or nt != tt * m or not 1 <= m <= PUSH_MAX_TOK:
            raise ValueError(f"StreamSenderNative.push: {na} audio and {nt} tactile samples; a push is {ta}*m and {tt}*m samples "
                             f"with one m, 1 <= m <= {PUSH_MAX_TOK} (anything else goes to finish)")
        with torch.no_grad():
            ya = self.rs[0].push(a.to(self.dev, torch.float32))
            yt = self.rs[1].push(t.to(self.dev, torch.float32))
        assert ya.shape == yt.shape and ya.shape[2] % HOP == 0
        if ya.shape[2] == 0:                                                           # the first token: the resamplers' lag
            return self.inner._nothing()
        return self.inner.push(ya, yt)

    def finish(self, a=None, t=None):
        """Flush (class docstring): the remaining native samples of either modality, or none -> the inner ``finish``'s tuple, with
        the packets, audio codes and parity of the inner pushes that preceded it in front, per item."""
        import torch
        self.inner._open("finish")
        a = None if a is None else self._native(a, "a", "finish")
        t = None if t is None else self._native(t, "t", "finish")
        with torch.no_grad():
            ya, yt = (y.reshape(self.batch, 1, y.shape[-1]) for y in
                      (rs.finish(None if x is None else x.to(self.dev, torch.float32)) for rs, x in zip(self.rs, (a, t))))
        T = min(ya.shape[2], yt.shape[2])                                              # crop_match
        outs, at = [], 0
        while T - at >= HOP:
            n = min((T - at) // HOP, PUSH_MAX_TOK) * HOP
            outs.append(self.inner.push(ya[:, :, at:at + n], yt[:, :, at:at + n]))
            at += n
        fin = self.inner.finish(ya[:, :, at:T], yt[:, :, at:T]) if T > at else self.inner.finish()
        n_info = 2 if self.inner.audio_packets else 1
        merged = list(fin)
        for i in range(len(fin) - n_info):                                             # push element i is finish element i, the infos skipped
            j = i if i < 2 else i + n_info
            parts = [o[i] for o in outs] + [fin[j]]
            if isinstance(fin[j], torch.Tensor):
                merged[j] = torch.cat(parts, dim=2)
            else:
                merged[j] = [sum((p[b] for p in parts), []) for b in range(self.batch)]
        return tuple(merged)


def _receiver_args(who, net, K, nb, packet_tok, conceal, out_rate):
    """What a receiver session refuses at construction, StreamReceiver and StreamReceiverPool alike."""
    from . import proposed
    from .packets import StreamInfo, _check
    if conceal == "plc":
        raise ValueError(f"{who}: conceal='plc' attends over the whole sequence and cannot run on a chunk")
    if conceal not in ("predict", "zero"):
        raise ValueError(f"{who}: conceal must be 'predict' or 'zero', not {conceal!r}")
    if packet_tok < 1 or CHUNK_TOK % packet_tok:
        raise ValueError(f"{who}: packet_tok = {packet_tok} does not divide the {CHUNK_TOK}-token chunk "
                         "(a packet must never straddle two chunks)")
    if K != net.vq.n_embed:
        raise ValueError(f"{who}: the stream has K = {K}, the model's codebook has {net.vq.n_embed}")
    if not 0 <= nb <= net.vq.n_books:
        raise ValueError(f"{who}: nb = {nb} books, the model has {net.vq.n_books}")
    if int(out_rate) not in (proposed.EVAL_SR, proposed.ORIG_3K):
        raise ValueError(f"{who}: out_rate must be {proposed.EVAL_SR} or {proposed.ORIG_3K}, not {out_rate}")
    assert proposed.AR_CHUNK_TOK == CHUNK_TOK
    _check(StreamInfo(K, nb, CHUNK_TOK, packet_tok))


class _ReceiverCore:
    """What StreamReceiver and StreamReceiverPool share: the configuration, the state buffers -- one row block per session,
    ``rows`` of them: carry [rows, C], hist [rows, C, 20], for out_rate=3000 the resampler's rs_state [rows, 105] and, for an
    audio_out_rate other than 24000, the audio resampler's ars_state [rows, hold*orig + width] -- the
    check of a chunk's audio codes, and THE device sequence of a step, written once.  With ``sl`` None a step works on every
    session of the buffers (the lockstep receiver); with ``sl`` = (slots, slots_dev), the host list of a group's slots and its
    int32 device copy, on those sessions of a pool: the same launches under another addressing (csrc/stream.hip), which is why a
    pool session computes what a solo one does."""

    def __init__(self, net, K, nb, packet_tok, rows, books_use, conceal, out_rate, audio=None, fec=None, audio_fec=None,
                 audio_conceal="zero", decoder="window", who="StreamReceiver", audio_out=False, audio_fade=None, audio_out_rate=LINK_SR):
        import torch
        from . import ops, proposed
        from .packets import StreamInfo, _check
        self.net, self.K, self.nb, self.packet_tok = net, K, nb, packet_tok
        self.ars_plan = native_out_plan(who, audio_out_rate, audio_out)                # ValueError before any session state exists
        self.audio_out_rate = int(audio_out_rate)
        if decoder not in ("window", "stateful"):
            raise ValueError(f"{who}: decoder must be 'window' or 'stateful', not {decoder!r}")
        self.decoder = decoder
        if audio_out or audio_fade is not None:                                        # ValueError before any session state exists
            net._audio_out_args(who, audio_out, audio_fade)
        if decoder == "stateful":
            _f32_only(f"{who}(decoder='stateful')")
            if tuple(net.T_DEC._desc[2]) != DEC_RATES or net.T_DEC._desc[4]:
                raise ValueError(f"{who}: decoder rates {tuple(net.T_DEC._desc[2])}; the stage plan is written for {DEC_RATES} "
                                 "without output_padding")
        if audio_conceal not in ("zero", "mask", "hold"):
            raise ValueError(f"{who}: audio_conceal must be 'zero', 'mask' or 'hold', not {audio_conceal!r}")
        if audio_conceal != "zero" and audio is None:
            raise ValueError(f"{who}: audio_conceal goes with audio=(K_a, na)")
        self.audio_conceal = audio_conceal
        if audio_fec is not None and audio is None:
            raise ValueError(f"{who}: audio_fec goes with audio=(K_a, na)")
        if fec is not None:
            net._fec_resolve(fec, K, nb, packet_tok)
        self.fec, self.audio_fec = fec, audio_fec
        self.audio = None                                                              # (K_a, na): the audio codes arrive as packets
        if audio is not None:
            _f32_only(who)
            K_a, na = (int(v) for v in audio)
            if K_a != net.A_QUANT.codebook_size or not 1 <= na <= net.A_QUANT.n_codebooks:
                raise ValueError(f"{who}: the audio stream has K = {K_a}, nb = {na}; the model's audio quantiser has "
                                 f"K = {net.A_QUANT.codebook_size} and {net.A_QUANT.n_codebooks} stages")
            _check(StreamInfo(K_a, na, CHUNK_TOK, packet_tok))
            self.audio = (K_a, na)
            if audio_fec is not None:
                net._fec_resolve(audio_fec, K_a, na, packet_tok, what="audio_fec")
        self.front = _RxFront(K, nb, packet_tok, self.audio, fec, audio_fec)           # the upload's format, host and device side
        self.books_use, self.conceal, self.out_rate = books_use, conceal, int(out_rate)
        self.dev = net.proj_up.weight.device
        self.C = net.proj_up.out_channels
        self.n_audio_books = net.A_QUANT.n_codebooks
        self.carry = torch.zeros(rows, self.C, device=self.dev)                        # per session: z_run[..., -1] of the chunk before
        self.qa_carry = torch.zeros(rows, self.C, device=self.dev) if audio_conceal == "hold" else None   # the last held audio token
        self.hist = self.dec_state = None
        if decoder == "window":
            self.hist = torch.zeros(rows, self.C, 2 * DEC_HALO_TOK, device=self.dev)   # per session: the last <= 20 latent tokens
        else:                                                                          # per session: every decoder stage's tail (section 23)
            self.dec_state = net.T_DEC.stream_state(rows)
        # the audio output (section 27): a second decoder state fed with qa -- hist [rows, C, 20] or the audio decoder's stage tails --
        # and the fade's run lengths [rows, 11]; audio_out=False allocates nothing and launches nothing
        self.audio_out, self.audio_fade = bool(audio_out), audio_fade
        self.a_hist = self.a_dec_state = self.fade_state = None
        if self.audio_out:
            if decoder == "window":
                self.a_hist = torch.zeros(rows, self.C, 2 * DEC_HALO_TOK, device=self.dev)
            else:
                self.a_dec_state = net.audio_decoder.stream_state(rows)
            if audio_fade is not None and self.audio is not None:         # codes that arrive as codes lose nothing: no fade
                self.fade_state = ops.audio_fade_state(rows, self.dev)
        self.rs_state = self.rs_kernel = None
        if self.out_rate != proposed.EVAL_SR:
            from .resample import sinc_resample_kernel
            kern, width, orig, new = sinc_resample_kernel(proposed.EVAL_SR, self.out_rate)
            assert (orig, width, new) == (RS_ORIG, RS_WIDTH, 1)
            self.rs_kernel = kern.to(self.dev)
            self.rs_state = ops.resample_stream_state(orig, width, rows, self.dev)
        # the audio output at the playback rate (section 32): a second resampler state behind the fade; 24000 allocates and launches nothing
        self.ars_state = self.ars_kernel = None
        if self.ars_plan is not None:
            from .resample import sinc_resample_kernel
            kern, width, orig, new = sinc_resample_kernel(LINK_SR, self.audio_out_rate)
            assert (orig, new, width) == self.ars_plan[:3]
            self.ars_kernel = kern.to(self.dev)
            self.ars_state = ops.resample_stream_rational_state(orig, width, rows, self.dev)

    def _codes(self, audio_codes, n_lo, n_hi, sid=None):
        """A chunk's audio codes, checked: int [B, n_codebooks, n] for the lockstep receiver (``sid`` None), [n_codebooks, n] or
        [1, n_codebooks, n] (-> [n_codebooks, n]) for session ``sid`` of a pool; n_lo <= n <= n_hi."""
        import torch
        codes = torch.as_tensor(audio_codes)
        if sid is None:
            who, want = "StreamReceiver", f"[B={self.carry.shape[0]}, n_codebooks, tokens]"
            shape_ok = codes.dim() == 3 and codes.shape[0] == self.carry.shape[0]
        else:
            who, want = f"{self._who}: session {sid}", "[n_codebooks, tokens] or [1, n_codebooks, tokens]"
            if codes.dim() == 3 and codes.shape[0] == 1:
                codes = codes[0]
            shape_ok = codes.dim() == 2
        if not shape_ok or codes.dtype.is_floating_point or codes.dtype == torch.bool:
            raise ValueError(f"{who}: audio_codes must be int {want}, got {codes.dtype} {tuple(torch.as_tensor(audio_codes).shape)}")
        if codes.shape[-2] != self.n_audio_books:
            raise ValueError(f"{who}: {codes.shape[-2]} audio code rows, the model's quantiser has {self.n_audio_books}")
        if not n_lo <= codes.shape[-1] <= n_hi:
            want = f"{n_lo}" if n_lo == n_hi else f"{n_lo}..{n_hi}"
            raise ValueError(f"{who}: {codes.shape[-1]} audio tokens for a chunk of {want} tokens")
        return codes

    def _layout(self, G, n):
        """The front end's layout of ``G`` items of ``n`` tokens for this session's streams."""
        return self.front.layout(G, n)

    # ------------------------------------------------------------------------------------------------ the device sequence
    def _latents(self, up, codes, n, sl=None, last=False):
        """Device: the upload (a segment of the front end's layout) and codes [G, 32, n] -> indices -> latents [G, C, n].  The carried
        token moves on in place; for slots through a dense [G, C] copy, not written back for sessions that end (``last``: the
        next open() resets the slot).  With audio_out: -> (z, qa, nav), the audio latent as the predictor saw it and the chunk's
        per-token stage counts (None when the codes arrived as codes: nothing of them is ever lost)."""
        from . import ops
        G = (self.carry.shape[0] if codes is None else codes.shape[0]) if sl is None else len(sl[0])
        idx, nbv, acodes, nav = self.front.unpack(up, self._layout(G, n), G, n)
        if self.audio is not None:                            # the audio codes arrived as packets
            assert codes is None
            codes = acodes
        carry = self.carry if sl is None else ops.stream_rows(self.carry, sl[0], slots_dev=sl[1])
        want_qa = {"return_qa": True} if self.audio_out else {}
        if self.audio_conceal == "zero":
            z = self.net.decode_latents(codes, idx, books_use=self.books_use, nb_valid=nbv, z_prev=carry, z_last_out=carry, na_valid=nav,
                                        **want_qa)
        else:                                                 # "mask" is stateless per chunk; "hold" moves qa_carry on in place
            z = self.net.decode_latents(codes, idx, books_use=self.books_use, nb_valid=nbv, z_prev=carry, z_last_out=carry, na_valid=nav,
                                        audio_conceal=self.audio_conceal, qa_prev=self.qa_carry, qa_last_out=self.qa_carry,
                                        **({} if sl is None or self.qa_carry is None else {"qa_slots": sl[0], "qa_slots_dev": sl[1]}),
                                        **want_qa)
        qa = None
        if self.audio_out:
            z, qa = z
        if sl is not None and not last:
            ops.stream_rows(self.carry, sl[0], rows=carry, slots_dev=sl[1])
        if self.conceal == "zero":                            # the post-pass of decode_latents(conceal="zero"), after the carry
            z = ops.plc_mask_fill(z, None, nbv == 0)[0]
        return (z, qa, nav) if self.audio_out else z

    def _window_decode(self, z, h_in, h_out, e0, e1, sl=None, last=False, audio=False):
        """Device: window = [history | z] (history updated in place), T_DEC on it, samples [e0, e1) of the window's output.
        decoder="stateful": the same samples from T_DEC.forward_stream, every stage on [its tail | its new columns] (dec_state updated
        in place).  h_in = min(tokens_before, 20) stands for tokens_before there: the stage plan depends on it only through
        min(tokens_before, 16).  ``audio``: the same plan on the audio branch -- z is qa, the decoder the attached audio decoder, the
        state a_hist / a_dec_state."""
        from . import ops
        dec, hist, dec_state = (self.net.audio_decoder, self.a_hist, self.a_dec_state) if audio else (self.net.T_DEC, self.hist, self.dec_state)
        if dec_state is not None:
            y = dec.forward_stream(dec_state, z, h_in, last, slots=None if sl is None else sl[0],
                                   slots_dev=None if sl is None else sl[1])
            assert y.shape[-1] == e1 - e0
            return y
        if sl is None:
            win = ops.stream_window(hist, h_in, z, h_out)
        else:
            win = ops.stream_window_slots(hist, sl[0], h_in, z, h_out, slots_dev=sl[1])
        return dec(win)[..., e0:e1]

    def _audio_step(self, qa, nav, h_in, h_out, e0, e1, sl, last):
        """Device, behind the tactile decode and on its stream: the same window plan / stage plan on qa through the audio decoder,
        then the fade in place on the emitted piece (ops.audio_fade_; fade_state moves on).  The piece starts at token
        max(0, tokens_before - 10); the fade launch depends on that only through "is it 0", which min(tokens_before, 20) = h_in tells.
        A session whose codes arrive as codes (audio=None) loses nothing and has no fade state: no fade launch."""
        from . import ops
        y = self._window_decode(qa, h_in, h_out, e0, e1, sl, last, audio=True).contiguous()
        if self.fade_state is not None and y.shape[-1] > 0:
            ops.audio_fade_(y, nav, self.fade_state, self.audio_fade, max(0, h_in - DEC_HALO_TOK),
                            slots=None if sl is None else sl[0], slots_dev=None if sl is None else sl[1])
        return y

    def _device_step(self, up, codes, n, h_in, h_out, e0, e1, sl=None, last=False):
        """A step up to the emit slice -> y [G, 1, e1 - e0].  n = 0 (a finish without a partial chunk) decodes the history alone;
        without a history either (a session that never got a token) nothing runs.  With audio_out -> (y, y_audio), the audio
        branch (``_audio_step``) after the tactile one, one after the other on the one stream."""
        import torch
        G = self.carry.shape[0] if sl is None else len(sl[0])
        if h_in + n == 0:
            y = torch.empty(G, 1, 0, device=self.dev)
            return (y, torch.empty(G, 1, 0, device=self.dev)) if self.audio_out else y
        z = self._latents(up, codes, n, sl, last) if n else torch.empty(G, self.C, 0, device=self.dev)
        if not self.audio_out:
            return self._window_decode(z, h_in, h_out, e0, e1, sl, last)
        z, qa, nav = z if n else (z, torch.empty(G, self.C, 0, device=self.dev), None)
        y = self._window_decode(z, h_in, h_out, e0, e1, sl, last)
        return y, self._audio_step(qa, nav, h_in, h_out, e0, e1, sl, last)

    def _decimate(self, y, consumed, last, sl=None):
        """out_rate=3000: the emitted piece through the streamed resampler, ``consumed`` = the samples the sessions emitted before
        (a pool group's launch class).  An empty piece -- the finish of a session without a token -- launches nothing."""
        from . import ops
        G, n = y.shape[0], y.shape[-1]
        if self.rs_state is None or n == 0:
            return y
        if sl is None:
            y3 = ops.resample_stream(y.reshape(G, n), self.rs_kernel, self.rs_state, consumed, RS_ORIG, 1, RS_WIDTH, final=last)
        else:
            y3 = ops.resample_stream_slots(y.reshape(G, n), self.rs_kernel, self.rs_state, sl[0], consumed, RS_ORIG, 1, RS_WIDTH,
                                           final=last, slots_dev=sl[1])
        return y3.unsqueeze(1)

    def _audio_rate(self, ya, consumed, last, sl=None):
        """audio_out_rate: the emitted audio piece, behind ``_audio_step`` and so behind the fade, through the rational streamed
        resampler (ars_state moves on) -- ``_decimate``'s contract: ``consumed`` = the 24 kHz samples emitted before, 0 or at least
        1920 and so a launch class of a pool group; every piece but the last is whole tokens, so whole filter blocks.  The form
        comes from the sessions of the launch (audio_resample_form).  An empty piece launches nothing."""
        from . import ops
        G, n = ya.shape[0], ya.shape[-1]
        if self.ars_state is None or n == 0:
            return ya
        orig, new, width, hold, _ = self.ars_plan
        form = audio_resample_form(G)
        if sl is None:
            y = ops.resample_stream_rational(ya.reshape(G, n), self.ars_kernel, self.ars_state, consumed, orig, new, width, hold=hold,
                                             final=last, form=form)
        else:
            y = ops.resample_stream_rational_slots(ya.reshape(G, n), self.ars_kernel, self.ars_state, sl[0], consumed, orig, new, width,
                                                   hold=hold, final=last, slots_dev=sl[1], form=form)
        return y.unsqueeze(1)


class StreamReceiver(_ReceiverCore):
    """A receiver session for ``batch`` items advancing in lockstep: ``push`` one 16-token chunk at a time (whatever tactile
    packets of it arrived, and its audio codes), get back the samples that chunk completes; ``finish`` flushes.

    ``cat(pushes + [finish])`` equals ``decompress_packets`` on the same packets bit for bit (length 320*T - 8), for
    ``ops.get_arith() == "f32"``: the opt-in arithmetic modes scale per item, so a window changes their arithmetic and no equality
    is claimed for them.  A push returns the samples up to 10 tokens (the decoder look-ahead) before the newest token, so the
    algorithmic latency is one chunk plus the halo, 213.3 + 133.3 ms, instead of the whole item.

    ``push`` runs, in order: _RxFront.gather_item(seq_base=) and .fill per item -> ONE upload, the front end's segment for the batch
    (what it holds and where: _RxFront) -> _RxFront.unpack -> decode_latents(nb_valid=, z_prev=carry, z_last_out=carry) ->
    ops.stream_window (window = history | new latents; history updated in place) -> T_DEC on the window -> the emit slice (->
    ops.resample_stream for out_rate=3000):
    _ReceiverCore's sequence.  All session state is in fixed device buffers (carry [B, C], history [B, C, 20], rs_state [B, 105]).

    ``graph=True``: the steady step (36-token window, from the third push on) is captured once as a graph on one stream and
    replayed for every later chunk after the host has written the packet bodies and audio codes into the static upload buffers;
    the first two pushes and ``finish`` run eagerly, and so does the resampler launch.  THE TENSOR A PUSH RETURNS IS THEN A VIEW OF
    THE GRAPH'S OUTPUT BUFFER: it is valid until the next push (clone it to keep it).

    ``audio=(K_a, na)``: the audio codes arrive as layered packets too (StreamSender(audio="packets"), compress_packets_av):
    ``push(tactile_packets, audio_packets=...)`` and ``finish(tactile_packets, audio_packets=..., tokens=n)`` (the second
    positional argument means the same) gather both streams, both go
    up in the ONE upload, both are unpacked on the device and the per-token stage counts go into the chunk's from_codes
    (decode_latents(na_valid=)); the steady step stays one captured graph with static body and count buffers.  The concatenated
    output equals decompress_packets_av on the same packets.  ``audio=None``: today's behaviour exactly.

    ``audio_conceal`` ("zero" / "mask" / "hold", only with ``audio=``; decode_latents): what the predictor does with an audio token
    no stage of which arrived.  "mask" is stateless per chunk; "hold" adds one fixed device buffer qa_carry [B, C] to the session
    state -- the last held audio token, zero at the start, moved on in place by every chunk -- so the hold crosses chunk borders as
    it does in decompress_packets_av(audio_conceal=).  The steady step stays ONE captured graph whose only input is the static
    upload buffer.  "zero": today's behaviour exactly.

    ``fec`` / ``audio_fec`` (packets.Fec, the sender's; ``audio_fec`` needs ``audio=``; both None: today's behaviour exactly):
    ``push(..., fec_packets=, audio_fec_packets=)`` and ``finish(...)`` likewise take, per item, whatever parity packets of the chunk
    arrived (None: none did).  The front end gathers them (packets.gather_fec(seq_base=the chunk's first group) per item) behind
    the existing arrays of the ONE upload and runs ops.fec_recover in place ahead of each stream's unpack: recovery is inside the captured
    steady step, whose only input stays the static upload buffer, so the graph replays under any loss pattern.  A parity packet of
    an earlier chunk is counted in ``late`` and ignored, as a late data packet is.  The concatenated output equals
    decompress_packets(fec=) / decompress_packets_av(fec=, audio_fec=) on the same packets.

    ``decoder="stateful"`` (the default "window" is the sequence above, launch for launch): instead of T_DEC on
    the 36-token window, T_DEC.forward_stream -- every decoder stage keeps the tail of its own input in dec_state [B, S] (it replaces
    the history [B, C, 20]) and computes only its new columns.  Every push / finish returns exactly the window mode's tensor; the
    steady step stays ONE captured graph; everything in front of the latents and behind the samples is untouched.

    ``audio_out=True`` (needs net.set_audio_decoder; False: everything above, launch for launch): ``push`` and
    ``finish`` return (y_tactile, y_audio).  y_audio [B, 1, n] is the audio waveform of the same samples at 24 kHz (``out_rate``
    acts on the tactile output only): after the tactile decode the step runs the same window plan (a second history a_hist
    [B, C, 20]) or stage plan (a second a_dec_state) on qa, the audio latent the predictor saw, through the audio decoder, on the
    same stream.  ``audio_fade`` (packets.AudioFade): with ``audio=(K_a, na)`` the emitted piece then goes through ops.audio_fade_,
    whose state fade_state [B, 11] carries the loss runs across chunks.  The concatenated y_audio equals
    decompress_packets_av(audio_out=True, audio_fade=)'s.  With graph=True the steady step stays ONE captured graph, with two
    output buffers.

    ``audio_out_rate`` (24000: everything above, launch for launch; needs audio_out=True): y_audio leaves at
    that rate instead -- 44100, 48000, 22050, ... whatever ``native_out_plan`` admits.  The emitted 24 kHz piece goes, behind the
    fade, through ops.resample_stream_rational on a second resampler state ars_state [B, hold*orig + width] (87 samples for
    44.1 kHz), in the form ``audio_resample_form`` names for the batch, eagerly behind the captured step as the 3 kHz decimator
    runs.  The concatenated y_audio equals Resample(24000, audio_out_rate) of decompress_packets_av(audio_out=True)'s bit for bit;
    a push returns the outputs its samples complete, ceil(width/orig) filter blocks behind them."""

    def __init__(self, net, K, nb, packet_tok=2, batch=1, books_use=None, conceal="predict", out_rate=24000, graph=False, audio=None,
                 fec=None, audio_fec=None, audio_conceal="zero", decoder="window", audio_out=False, audio_fade=None, audio_out_rate=24000):
        K, nb, packet_tok, batch = int(K), int(nb), int(packet_tok), int(batch)
        _receiver_args("StreamReceiver", net, K, nb, packet_tok, conceal, out_rate)
        if batch < 1:
            raise ValueError("StreamReceiver: batch must be at least 1")
        if fec is not None or audio_fec is not None:
            _f32_only("StreamReceiver")
        super().__init__(net, K, nb, packet_tok, batch, books_use, conceal, out_rate, audio=audio, fec=fec, audio_fec=audio_fec,
                         audio_conceal=audio_conceal, decoder=decoder, audio_out=audio_out, audio_fade=audio_fade,
                         audio_out_rate=audio_out_rate)
        self.batch, self.graph = batch, bool(graph)
        self.h = 0                                                                     # valid columns of hist
        self.tokens = 0                                                                # tokens received (N)
        self.late = 0                                                                  # packets of chunks already decoded
        self.finished = False
        self._g = None                                                                 # (graph, up_static, codes_static, y_static)

    # ------------------------------------------------------------------------------------------------------------ stages
    def _gather(self, tactile_packets, n, audio_packets=None, fec_packets=None, audio_fec_packets=None):
        """Host: per item whatever packets of this chunk arrived -> one uint8 array, the front end's segment for the batch
        (_RxFront.gather_item and .fill per item, against the session's sequence number)."""
        import numpy as np
        B, lay = self.batch, self._layout(self.batch, n)
        audio, fec, afec = ([None] * B if pk is None else self._packets_ok(pk)        # before anything is gathered
                            for pk in (audio_packets, fec_packets, audio_fec_packets))
        host, late = np.empty(lay.size, np.uint8), []
        for b in range(B):
            self.front.fill(host, lay, b, self.front.gather_item(tactile_packets[b], audio[b], fec[b], afec[b], n,
                                                                 seq_base=self.tokens // self.packet_tok, late=late))
        self.late += len(late)
        return host

    def _plan(self, n, last):
        """(h_in, h_out, e0, e1) of the step that takes n new tokens: schedule()'s step in window-local samples."""
        assert self.h == min(self.tokens, 2 * DEC_HALO_TOK)
        return _window_plan(self.tokens, n, last)

    def _packets_ok(self, tactile_packets):
        tactile_packets = list(tactile_packets)
        if len(tactile_packets) != self.batch:
            raise ValueError(f"StreamReceiver: packets of {len(tactile_packets)} items for a session of batch {self.batch}")
        return tactile_packets

    # ------------------------------------------------------------------------------------------------------------ session
    def _fec_args(self, what, fec_packets, audio_fec_packets):
        if (fec_packets is not None and self.fec is None) or (audio_fec_packets is not None and self.audio_fec is None):
            raise ValueError(f"StreamReceiver.{what}: fec_packets / audio_fec_packets need a session opened with fec= / audio_fec=")

    def push(self, tactile_packets, audio_codes=None, *, audio_packets=None, fec_packets=None, audio_fec_packets=None):
        """One chunk: ``tactile_packets`` = ``batch`` iterables of the packets of chunk c that arrived (the stream's sequence
        numbers [c*16/packet_tok, (c+1)*16/packet_tok); missing, reordered, duplicated or thinned), ``audio_codes`` int [B, 32, 16].
        -> y [B, 1, n_emit] (1920 samples for the first push, then 5120; a third of that at out_rate=3000, less the resampler's
        look-ahead).  A packet of an earlier chunk is counted in ``late`` and ignored; one of a later chunk raises ValueError.
        With graph=True the result is valid until the next push."""
        import torch
        from ._lib import MvqError
        if self.finished:
            raise MvqError("StreamReceiver: push after finish")
        audio_codes = self._audio_arg("push", audio_codes, audio_packets)
        self._fec_args("push", fec_packets, audio_fec_packets)
        if audio_codes is None:
            raise ValueError("StreamReceiver.push: a chunk needs its audio " + ("packets" if self.audio is not None else "codes"))
        tactile_packets = self._packets_ok(tactile_packets)
        n = CHUNK_TOK
        if self.audio is not None:                                            # the chunk's audio PACKETS
            host, codes = self._gather(tactile_packets, n, self._packets_ok(audio_codes), fec_packets, audio_fec_packets), None
        else:
            codes = self._codes(audio_codes, CHUNK_TOK, CHUNK_TOK)
            host = self._gather(tactile_packets, n, None, fec_packets)
        plan = self._plan(n, False)
        consumed = HOP * max(0, self.tokens - DEC_HALO_TOK)                   # the samples emitted so far
        with torch.no_grad():
            if self.graph and plan[0] == 2 * DEC_HALO_TOK:                    # the steady step: a full history
                y = self._replay(host, codes, n, plan)
            else:
                y = self._device_step(torch.from_numpy(host).to(self.dev), None if codes is None else codes.to(self.dev), n, *plan)
            self.h, self.tokens = plan[1], self.tokens + n
            if self.audio_out:
                return self._decimate(y[0], consumed, False), self._audio_rate(y[1], consumed, False)
            return self._decimate(y, consumed, False)

    def _audio_arg(self, what, audio_codes, audio_packets):
        """The audio side of a chunk: ``audio_codes`` (a tensor; sessions with audio=None) or ``audio_packets`` (per item the
        packets that arrived; sessions with audio=(K_a, na), where the second positional argument means the same)."""
        if audio_packets is None:
            return audio_codes
        if self.audio is None:
            raise ValueError(f"StreamReceiver.{what}: audio_packets needs a session opened with audio=(K_a, na)")
        if audio_codes is not None:
            raise ValueError(f"StreamReceiver.{what}: audio_packets or audio_codes, not both")
        return audio_packets

    def finish(self, tactile_packets=None, audio_codes=None, tokens=None, *, audio_packets=None, fec_packets=None, audio_fec_packets=None):
        """Flush: optionally a last partial chunk of 1..15 tokens (its packets and audio_codes [B, 32, n]; with audio=(K_a, na)
        its packets of both streams and ``tokens`` = n, which no lost packet can tell), then every remaining sample up to
        320*T - 8.  Runs eagerly.  The session accepts nothing afterwards."""
        import torch
        from ._lib import MvqError
        if self.finished:
            raise MvqError("StreamReceiver: finish after finish")
        audio_codes = self._audio_arg("finish", audio_codes, audio_packets)
        self._fec_args("finish", fec_packets, audio_fec_packets)
        if (tactile_packets is None) != (audio_codes is None):
            raise ValueError("StreamReceiver.finish: the last chunk needs both its packets and its audio codes")
        if tokens is not None and (self.audio is None or audio_codes is None):
            raise ValueError("StreamReceiver.finish: tokens= counts a last chunk of audio PACKETS (a session with audio=(K_a, na)); "
                             "audio codes carry their own length")
        n, up, codes = 0, None, None
        if audio_codes is not None and self.audio is not None:
            if tokens is None or not 1 <= int(tokens) <= CHUNK_TOK - 1:
                raise ValueError(f"StreamReceiver.finish: tokens = {tokens!r}; a last chunk of audio packets has 1..{CHUNK_TOK - 1} tokens")
            n = int(tokens)
            host = self._gather(self._packets_ok(tactile_packets), n, self._packets_ok(audio_codes), fec_packets, audio_fec_packets)
        elif audio_codes is not None:
            tactile_packets = self._packets_ok(tactile_packets)
            codes = self._codes(audio_codes, 1, CHUNK_TOK - 1)
            n = int(codes.shape[2])
            host = self._gather(tactile_packets, n, None, fec_packets)
        plan = self._plan(n, True)
        consumed = HOP * max(0, self.tokens - DEC_HALO_TOK)
        with torch.no_grad():
            if n:
                up, codes = torch.from_numpy(host).to(self.dev), None if codes is None else codes.to(self.dev)
            y = self._device_step(up, codes, n, *plan, last=True)
            self.h, self.tokens, self.finished = plan[1], self.tokens + n, True
            if self.audio_out:
                return self._decimate(y[0], consumed, True), self._audio_rate(y[1], consumed, True)
            return self._decimate(y, consumed, True)

    def _replay(self, host, codes, n, plan):
        """The steady step as a graph: captured at its first use (after one eager run at that shape on copies of the state, so
        that nothing is built during the capture), then replayed with the inputs written into the static buffers."""
        import torch
        if self._g is None:
            up_s = torch.from_numpy(host).to(self.dev)
            codes_s = None if codes is None else codes.to(self.dev).long().clone()
            state = (self.hist if self.dec_state is None else self.dec_state, self.carry) + \
                ((self.qa_carry,) if self.qa_carry is not None else ()) + \
                tuple(t for t in (self.a_hist, self.a_dec_state, self.fade_state) if t is not None)
            g, y_s = _capture(self.dev, state, lambda: self._device_step(up_s, codes_s, n, *plan))
            self._g = (g, up_s, codes_s, y_s)
            if self.fec is not None or self.audio_fec is not None:            # the eager run before the capture recovered in place
                up_s.copy_(torch.from_numpy(host))
        else:
            g, up_s, codes_s, y_s = self._g
            up_s.copy_(torch.from_numpy(host))
            if codes_s is not None:
                codes_s.copy_(codes)
        g.replay()
        return y_s


class PoolChunk(NamedTuple):
    """What StreamReceiverPoolAV.step takes for one session of a tick: the chunk's tactile packets that arrived, its ``audio`` --
    the audio packets that arrived for a pool opened with audio=(K_a, na), else the audio codes int [32, n] -- then, for a pool
    opened with fec= / audio_fec=, the parity packets of each stream that arrived (None: none did); ``tokens`` (1..15) belongs to
    a finish whose audio travels as packets, as StreamReceiver.finish(tokens=).  A plain tuple of the first 2..5 values does too.
    StreamReceiverPool.step takes exactly the first two values."""
    tactile_packets: object
    audio: object
    fec_packets: object = None
    audio_fec_packets: object = None
    tokens: object = None


class StreamReceiverPool(_SessionTable, _ReceiverCore):
    """Receiver sessions that join, run for different lengths and leave independently, served together: ``open`` takes a
    session slot, ``step`` is one tick that advances whichever sessions have a chunk ready (and flushes the ones that end),
    ``close`` abandons one.  Every session gets back exactly what a ``StreamReceiver(batch=1)`` fed the same data returns from
    ``push`` / ``finish``, bit for bit (``ops.get_arith() == "f32"`` only, as there).

    The state of all ``slots`` sessions lies in one set of device buffers allocated once -- carry [S, C], hist [S, C, 20] and, for
    out_rate=3000, the resampler's [S, 105] -- and a session is a row block of each (its slot).  A tick runs, in order:
      host   every session's input checked and gathered (_RxFront.gather_item against ITS seq_base, the audio codes' shape, the
             sids); an error leaves every session as it was, the late counters too;
             pool_groups: the sessions that share a launch sequence -- at most three groups of pushes (first, second, steady
             chunk), one more per kind of finisher;
      copy   ONE upload of all groups' slot lists and then per group ONE segment of the front end's layout (_RxFront.fill
             session by session: here the packet bodies and counts), ONE of all audio codes;
      device per group of G sessions: _RxFront.unpack -> ops.stream_rows (the carried tokens, pool -> dense [G, C]) ->
             decode_latents(z_prev=, z_last_out=) -> ops.stream_rows back -> ops.stream_window_slots -> T_DEC on [G, C, window]
             -> the emit slice (-> ops.resample_stream_slots): _ReceiverCore's sequence on the group's slots.
    ``step`` reads nothing back from the device.  Nothing is captured as a graph: the group sizes change from tick to tick.

    ``decoder="stateful"``: as for StreamReceiver -- dec_state [S, floats] replaces hist, and a group's decode is
    T_DEC.forward_stream on the group's slots.  ``open`` leaves a slot's dec_state as it is: a new session reads no tail."""

    _who = "StreamReceiverPool"
    _item_fields = 2                                                                   # an item is (packets, audio_codes), no more

    def __init__(self, net, K, nb, packet_tok=2, slots=64, books_use=None, conceal="predict", out_rate=24000, audio_conceal=None,
                 decoder="window", audio_out=False, audio_fade=None):
        if audio_conceal is not None:
            raise ValueError("StreamReceiverPool: the pool takes no audio= packets and so no audio_conceal")
        if audio_out or audio_fade is not None:
            raise ValueError("StreamReceiverPool: the pool has no audio output; audio_out / audio_fade go with StreamReceiverPoolAV")
        self._init_pool(net, K, nb, packet_tok, slots, books_use, conceal, out_rate, decoder=decoder)

    def _init_pool(self, net, K, nb, packet_tok, slots, books_use, conceal, out_rate, **options):
        """What both receiver pools' constructors do: the refusals, _ReceiverCore's buffers with ``slots`` rows, an empty session
        table (sid -> [slot, tokens, late])."""
        K, nb, packet_tok, slots = int(K), int(nb), int(packet_tok), int(slots)
        _receiver_args(self._who, net, K, nb, packet_tok, conceal, out_rate)
        if slots < 1:
            raise ValueError(f"{self._who}: slots must be at least 1")
        _f32_only(self._who)
        super().__init__(net, K, nb, packet_tok, slots, books_use, conceal, out_rate, **options)
        self._init_sessions(slots)

    # ----------------------------------------------------------------------------------------------------------- sessions
    def tokens(self, sid):
        """Tokens session ``sid`` has received."""
        return self._get(sid, "tokens")[1]

    def late(self, sid):
        """Packets of chunks already decoded that session ``sid`` was handed (counted and ignored)."""
        return self._get(sid, "late")[2]

    def open(self):
        """A new session -> its sid (never reused).  Takes the lowest free slot and resets it: the carried token and the
        resampler state to zero on the device, the history count (the session's tokens) to zero."""
        slot = self._take_slot()
        self.carry[slot].zero_()
        if self.qa_carry is not None:                                                  # StreamReceiverPoolAV(audio_conceal="hold")
            self.qa_carry[slot].zero_()
        if self.rs_state is not None:
            self.rs_state[slot].zero_()
        if self.ars_state is not None:                                                 # StreamReceiverPoolAV(audio_out_rate=)
            self.ars_state[slot].zero_()
        return self._new_session(slot, 0, 0)

    # --------------------------------------------------------------------------------------------------------------- tick
    def _inputs(self, pushes, finishes):
        """Host: every session's input of this tick, checked and gathered; raises before anything has changed.
        -> {sid: (n, last, parts, codes [32, n] or None, late packets)}; ``parts``: the session's arrays in the front end's layout
        order (_RxFront.gather_item: bodies, counts[, audio bodies, audio counts][, rows, got per stream with a Fec]) or None."""
        who, work = self._who, {}
        for sid in pushes:
            if sid in finishes:
                raise ValueError(f"{who}: session {sid!r} is both pushed and finished in one tick")
        audio_what = "audio_packets" if self.audio is not None else "audio_codes"
        item_what = f"(packets, {audio_what}" + (")" if self._item_fields == 2 else "[, fec_packets, audio_fec_packets[, tokens]])")
        for last, items in ((False, pushes), (True, finishes)):
            for sid, item in items.items():
                tokens = self._get(sid, "finish" if last else "push")[1]
                if item is None:
                    if not last:
                        raise ValueError(f"{who}: session {sid}: a push needs (packets, {audio_what})")
                    work[sid] = (0, True, None, None, 0)
                    continue
                try:
                    item = tuple(item)
                    if len(item) > self._item_fields:
                        raise TypeError
                    item = PoolChunk(*item)
                except TypeError:
                    raise ValueError(f"{who}: session {sid}: {item_what} expected") from None
                if item.tactile_packets is None or item.audio is None:
                    raise ValueError(f"{who}: session {sid}: a chunk needs both its packets and its {audio_what}")
                if (item.fec_packets is not None and self.fec is None) or (item.audio_fec_packets is not None and self.audio_fec is None):
                    raise ValueError(f"{who}: session {sid}: fec_packets / audio_fec_packets need a pool opened with fec= / audio_fec=")
                codes = None
                if self.audio is not None:
                    if not last:
                        if item.tokens is not None:
                            raise ValueError(f"{who}: session {sid}: tokens= belongs to a finish; a push is a {CHUNK_TOK}-token chunk")
                        n = CHUNK_TOK
                    elif item.tokens is None or not 1 <= int(item.tokens) <= CHUNK_TOK - 1:
                        raise ValueError(f"{who}: session {sid}: tokens = {item.tokens!r}; a last chunk of audio packets has "
                                         f"1..{CHUNK_TOK - 1} tokens")
                    else:
                        n = int(item.tokens)
                else:
                    if item.tokens is not None:
                        raise ValueError(f"{who}: session {sid}: tokens= counts a last chunk of audio PACKETS (a pool with "
                                         "audio=(K_a, na)); audio codes carry their own length")
                    codes = self._codes(item.audio, 1, CHUNK_TOK - 1, sid) if last else self._codes(item.audio, CHUNK_TOK, CHUNK_TOK, sid)
                    n = int(codes.shape[1])
                late = []
                parts = self.front.gather_item(item.tactile_packets, item.audio, item.fec_packets, item.audio_fec_packets, n,
                                               seq_base=tokens // self.packet_tok, late=late)
                work[sid] = (n, last, parts, codes, len(late))
        return work

    def _upload(self, work):
        """Host: the tick's groups and its ONE uint8 array -- the slot lists of all groups (int32, first: aligned), then per group
        that takes tokens its segment in the front end's layout -> (groups, slot_lists, [(segment offset, RxLayout or None)], host)."""
        import numpy as np
        groups = pool_groups((sid, self._sess[sid][1], w[0], w[1]) for sid, w in work.items())
        size, where = 4 * sum(len(g.sids) for g in groups), []
        for g in groups:
            lay = self._layout(len(g.sids), g.key[1]) if g.key[1] else None
            where.append((size, lay))
            size += lay.size if lay is not None else 0
        host = np.empty(size, np.uint8)
        slot_lists = [[self._sess[sid][0] for sid in g.sids] for g in groups]
        host[:where[0][0]] = np.asarray([s for sl in slot_lists for s in sl], np.int32).view(np.uint8)
        for g, (o, lay) in zip(groups, where):
            for i, sid in enumerate(g.sids if lay is not None else ()):
                self.front.fill(host[o:o + lay.size], lay, i, work[sid][2])
        return groups, slot_lists, where, host

    def step(self, pushes, finishes=None):
        """One tick.  ``pushes``: {sid: (packets of its current chunk that arrived, audio_codes int [32, 16] or [1, 32, 16])};
        ``finishes``: {sid: (packets, audio_codes [32, n]) with 1 <= n <= 15, or None} for the sessions that end with this tick.
        -> {sid: y [1, 1, n_emit]}: per session what StreamReceiver(batch=1).push / .finish returns (views of the group's
        output).  A finished session's slot is freed.  ValueError / MvqError for any one session (a packet of a later chunk, a
        wrong code shape, an unknown sid, a sid in both maps) comes before the first device call and leaves every session as it
        was.  StreamReceiverPoolAV: an item is a PoolChunk or (packets, audio[, fec_packets[, audio_fec_packets]]) -- ``audio`` the
        chunk's audio packets (a pool with audio=(K_a, na)) or its audio codes; a last chunk of audio packets is PoolChunk(...,
        tokens=n); with audio_out a session's result is (y, y_audio); parity packets without the matching fec= and a missing
        tokens= are refused like the rest."""
        import torch
        pushes, finishes = dict(pushes or {}), dict(finishes or {})
        _f32_only(self._who)
        work = self._inputs(pushes, finishes)
        if not work:
            return {}
        groups, slot_lists, where, host = self._upload(work)
        flat_codes =[work[sid][3].reshape(-1) for g in groups if g.key[1] and self.audio is None for sid in g.sids]
        out = {}
        with torch.no_grad():
            up = torch.from_numpy(host).to(self.dev)
            if flat_codes:
                if any(c.is_cuda for c in flat_codes):
                    codes_all = torch.cat([c.to(self.dev, torch.int64) for c in flat_codes])
                else:
                    codes_all = torch.cat([c.to(torch.int64) for c in flat_codes]).to(self.dev)
            slots_all = up[:where[0][0]].view(torch.int32)                   # the slot lists lie in front of the first segment
            s0 = c0 = 0
            for g, slots, (o, lay) in zip(groups, slot_lists, where):
                G, (_, n, last) = len(g.sids), g.key
                sl = (slots, slots_all[s0:s0 + G])
                codes = None
                if n and self.audio is None:
                    codes = codes_all[c0:c0 + G * self.n_audio_books * n].view(G, self.n_audio_books, n)
                    c0 += G * self.n_audio_books * n
                seg = up[o:o + lay.size] if lay is not None else None
                y = self._device_step(seg, codes, n, *g.plan, sl=sl, last=last)
                y, ya = y if self.audio_out else (y, None)
                y = self._decimate(y, g.consumed, last, sl)
                if self.audio_out:
                    ya = self._audio_rate(ya, g.consumed, last, sl)
                s0 += G
                for i, sid in enumerate(g.sids):
                    out[sid] = (y[i:i + 1], ya[i:i + 1]) if self.audio_out else y[i:i + 1]
        for sid, w in work.items():
            if w[1]:
                self.close(sid)
            else:
                self._sess[sid][1] += w[0]
                self._sess[sid][2] += w[4]
        return out


class StreamSenderPool(_SessionTable, _SenderCore):
    """Sender sessions that join at any time, push 1..16 tokens of samples at a time and end after different lengths, served
    together: ``open`` takes a session slot, ``step`` is one tick that takes the samples of whichever sessions have some (and
    flushes the ones that end), ``close`` abandons one.  Every session gets back exactly what a ``StreamSender(batch=1)`` fed
    the same samples returns from ``push`` / ``finish`` (``ops.get_arith() == "f32"`` only, as there), so per session the
    packets concatenated equal ``compress_packets``' of that item alone byte for byte.

    The state of all ``slots`` sessions lies in device buffers allocated once -- buf [S, 2, 48*320] (a session's audio and tactile
    row) and carry [S, C] -- and a session is a row block of each (its slot); its (fill, start, chunk) are host integers.  A tick
    runs, in order:
      host   every session's samples checked (StreamSender's checks, the sids); an error leaves every session as it was;
             sender_step per session, sender_pool_groups: ONE group of the pushes that emit nothing, at most two of the pushes
             that emit (chunk 0: the 24-token window; later: the 32-token window), one more per kind of finisher -- inside a
             group every session has its own fill, n and drop;
      copy   ONE upload of all groups' descriptor tables and slot lists, ONE of all new samples (host tensors; samples already
             on the device are concatenated there);
      device per group of G sessions: ops.stream_samples_slots (per-session fill / n / drop, window [2, G, w] out, buffers moved
             on) -> A_ENC, T_ENC on [G, 1, w] -> tokens [lo, hi) -> A_QUANT -> ops.stream_rows (the carried tokens, pool -> dense
             [G, C]) -> _ar_latents(z_prev=, z_last_out=) -> ops.stream_rows back (not for a group that finishes: its slots are
             freed) -> _TxBack.pack: _SenderCore's sequence on the group's slots.  The append group is the sample-state launch alone;
      copy   ONE device-to-host copy of all groups' rows, then _TxBack.frame_item per session with ITS chunk's sequence base.
    Nothing is captured as a graph: the group sizes change from tick to tick.

    ``encoder="stateful"``: as for StreamSender -- enc_state (two [S, floats] buffers) beside the sample buffers, a group's encode is
    A_ENC / T_ENC.forward_stream on the group's slots, fed the members' un-encoded samples (``sender_pool_groups(stateful=True)``
    groups by what the stage plan depends on).  ``open`` leaves a slot's enc_state as it is: a new session reads no tail."""

    _who = "StreamSenderPool"

    def __init__(self, net, packet_tok=2, slots=64, books_use=None, encoder="window"):
        self._init_pool(net, packet_tok, slots, books_use, encoder=encoder)

    def _init_pool(self, net, packet_tok, slots, books_use, **options):
        """What both sender pools' constructors do: _SenderCore's checks and buffers with ``slots`` rows, an empty session table
        (sid -> [slot, fill, start, chunk])."""
        packet_tok, slots = int(packet_tok), int(slots)
        super().__init__(self._who, net, packet_tok, books_use, slots, (slots, 2, SEND_CAP_TOK * HOP), **options)
        self._init_sessions(slots)
        self.last_groups = ()                                                          # the SenderGroups of the last tick

    # ----------------------------------------------------------------------------------------------------------- sessions
    def tokens(self, sid):
        """Tokens of samples session ``sid`` has received."""
        _, fill, start, _ = self._get(sid, "tokens")
        return start + fill // HOP

    def open(self):
        """A new session -> its sid (never reused).  Takes the lowest free slot and resets it: the carried token to zero on the
        device, the fill to zero on the host (which makes whatever the slot's buffer rows hold irrelevant)."""
        slot = self._take_slot()
        self.carry[slot].zero_()
        return self._new_session(slot, 0, 0, 0)

    # --------------------------------------------------------------------------------------------------------------- tick
    def _inputs(self, pushes, finishes):
        """Host: every session's samples of this tick, checked; raises before anything has changed.
        -> {sid: (a [1, 1, n] or None, t or None, n, last)}"""
        work = {}
        for sid in pushes:
            if sid in finishes:
                raise ValueError(f"{self._who}: session {sid!r} is both pushed and finished in one tick")
        for last, items in ((False, pushes), (True, finishes)):
            for sid, item in items.items():
                fill = self._get(sid, "finish" if last else "push")[1]
                if item is None:
                    if not last:
                        raise ValueError(f"{self._who}: session {sid}: a push needs its samples (a, t)")
                    work[sid] = (None, None, 0, True)
                    continue
                try:
                    a, t = item
                except (TypeError, ValueError):
                    raise ValueError(f"{self._who}: session {sid}: the samples (a, t) of both modalities expected") from None
                a, t, n = _sender_samples(f"{self._who}: session {sid}", "finish" if last else "push", a, t, 1, fill, tail=last)
                work[sid] = (a, t, n, last)
        return work

    def step(self, pushes, finishes=None):
        """One tick.  ``pushes``: {sid: (a, t)}, the next samples [1, 1, 320*m] of both modalities, 1 <= m <= 16, m per session;
        ``finishes``: {sid: (a, t) of any length, or None} for the sessions that end with this tick.
        -> {sid: (packets, audio_codes)} for the pushes and {sid: (packets, audio_codes, StreamInfo)} for the finishes: the
        session's framed packets (a list of ``bytes``, numbered with ITS stream's sequence numbers) and int64 [1, 32, n] on the
        device -- what StreamSender(batch=1).push / .finish returns for its one item; an empty list and [1, 32, 0] when the
        push completes no chunk.  A finished session's slot is freed.  ValueError / MvqError for any one session (a push that is
        no 320*m samples, modalities of different length, an unknown sid, a sid in both maps) comes before the first device call
        and leaves every session as it was."""
        import numpy as np
        import torch
        from . import ops
        pushes, finishes = dict(pushes or {}), dict(finishes or {})
        _f32_only(self._who)
        work = self._inputs(pushes, finishes)
        if not work:
            return {}
        stateful = self.enc_state is not None
        groups = sender_pool_groups(((sid, *self._sess[sid][1:], w[2], w[3]) for sid, w in work.items()), stateful=stateful)
        steps = {sid: st for g in groups for sid, st in zip(g.sids, g.steps)}
        for sid, w in work.items():                                      # the finishers without a token: no device work
            if sid not in steps:
                steps[sid] = self._step(*self._sess[sid][1:], w[2], w[3])
        if stateful and any(g.w > ENC_STREAM_MAX_N for g in groups):
            raise ValueError(f"{self._who}: encoder='stateful' takes at most {ENC_STREAM_MAX_N} samples in one step")
        cap = self.buf.shape[2]
        # ONE host array: the descriptor tables of all groups (int32 [5] per session), then their slot lists
        tables = [ops.stream_samples_desc([(self._sess[sid][0], self._sess[sid][1], work[sid][2], st.drop)
                                           for sid, st in zip(g.sids, g.steps)], g.w, cap, self._who) for g in groups]
        n_sess = sum(len(g.sids) for g in groups)
        host = np.asarray([r for rows, _ in tables for r in rows], np.int32).reshape(n_sess, 5)
        host = np.concatenate([host.reshape(-1), host[:, 0]])
        pieces = [x.reshape(-1) for g in groups for sid in g.sids if work[sid][2] for x in work[sid][:2]]
        out, bodies_all, framing = {}, [], []
        with torch.no_grad():
            if groups:
                up = torch.from_numpy(host).to(self.dev)
                desc_all, slots_all = up[:5 * n_sess].view(n_sess, 5), up[5 * n_sess:]
                if not pieces:
                    x_all = torch.empty(0, device=self.dev)
                elif any(p.is_cuda for p in pieces):
                    x_all = torch.cat([p.to(self.dev, torch.float32) for p in pieces])
                else:
                    x_all = torch.cat([p.to(torch.float32) for p in pieces]).to(self.dev)
            s0 = x0 = b0 = 0
            for g, (rows, x_total) in zip(groups, tables):
                G = len(g.sids)
                win = ops.stream_samples_slots(self.buf, [r[:4] for r in rows], x_all[x0:x0 + x_total], g.w, desc_dev=desc_all[s0:s0 + G])
                if g.hi > g.lo:
                    # stateful: the stage plan is the same for every member (sender_pool_groups), so the first one's samples_before
                    bodies, codes = self._encode(win, g.lo, g.hi, sl=([r[0] for r in rows], slots_all[s0:s0 + G]),
                                                 before=HOP * self._sess[g.sids[0]][2] if stateful else None, last=g.key[0] == "finish")
                    bodies_all.append(bodies.reshape(-1))
                    per = bodies.numel() // G
                    for i, sid in enumerate(g.sids):
                        framing.append((sid, b0 + i * per, per, g.hi - g.lo, codes[i:i + 1]))
                    b0 += G * per
                s0, x0 = s0 + G, x0 + x_total
            if bodies_all:                                                # ONE device-to-host copy of the tick's packet bodies
                host_b = (bodies_all[0] if len(bodies_all) == 1 else torch.cat(bodies_all)).cpu().numpy()
        for sid, at, per, n_tok, codes in framing:
            out[sid] = self._frame(host_b[at:at + per], n_tok, self._sess[sid][3], codes)
        nothing = None
        for sid, w in work.items():
            st = steps[sid]
            if sid not in out:
                nothing = self._nothing() if nothing is None else nothing
                out[sid] = tuple([] if isinstance(v, list) else v for v in nothing)    # the empty codes tensor is shared
            if w[3]:                                                      # the StreamInfo(s) behind the two data elements
                out[sid] = self._finished(out[sid], self._sess[sid][2] + max(st.hi, 0))
                self.close(sid)
            else:
                self._sess[sid][1:] = [st.fill, st.start, st.chunk]
        self.last_groups = tuple(groups)
        return out


class StreamReceiverPoolAV(StreamReceiverPool):
    """StreamReceiverPool for the whole link: the options of StreamReceiver -- ``audio=(K_a, na)`` (the audio
    codes arrive as layered packets), ``fec`` / ``audio_fec``, ``audio_conceal``, beside ``conceal``, ``out_rate`` and ``decoder`` --
    with the same meaning and the same refusals.  Sessions are StreamReceiverPool's (open / close / active / free / tokens / late).
    Every session gets from ``step`` exactly what a ``StreamReceiver(batch=1)`` with the same options, fed the same data, returns
    from ``push`` / ``finish``, bit for bit.

    A tick IS StreamReceiverPool's -- the class adds its constructor and nothing else; the base class's ``step`` serves both and an
    item may carry all of PoolChunk's fields here.  The options only widen the group's segment, whose format the front end owns
    (_RxFront: tactile bodies, counts, audio bodies, counts, per stream the parity rows and their ``got`` flags); ONE upload of the
    slot lists and all segments (and ONE of the audio codes, for audio=None only); then per group _ReceiverCore's sequence on the
    group's slots: _RxFront.unpack (ops.fec_recover in place ahead of each stream's unpack), the carried token through
    ops.stream_rows, decode_latents -- "hold" addresses the held audio token qa_carry [S, C] through the slot list
    (ops.hold_fill_(slots=)) -- and the decode.  Nothing is read back.  ``open`` resets the slot's carried token, held audio token
    and resampler state.

    ``audio_out`` / ``audio_fade`` (StreamReceiver's): a session's result is (y_tactile, y_audio).  The pool
    holds a second decoder state (a_hist [S, C, 20] or a_dec_state) and the fade's run lengths fade_state [S, 11]; a group's step
    runs the audio branch on the group's slots after the tactile one.  ``open`` clears none of them: a new session reads no
    history, no tail and no run length.  ``audio_out_rate`` (StreamReceiver's; section 32): a group's audio piece goes through
    ops.resample_stream_rational_slots on the group's slots of ars_state [S, hold*orig + width], its launch class the group's
    ``consumed``; ``open`` zeroes the slot's row, as it zeroes rs_state's."""

    _who = "StreamReceiverPoolAV"
    _item_fields = len(PoolChunk._fields)

    def __init__(self, net, K, nb, packet_tok=2, slots=64, books_use=None, conceal="predict", out_rate=24000, audio=None, fec=None,
                 audio_fec=None, audio_conceal="zero", decoder="window", audio_out=False, audio_fade=None, audio_out_rate=24000):
        self._init_pool(net, K, nb, packet_tok, slots, books_use, conceal, out_rate, audio=audio, fec=fec, audio_fec=audio_fec,
                        audio_conceal=audio_conceal, decoder=decoder, who=self._who, audio_out=audio_out, audio_fade=audio_fade,
                        audio_out_rate=audio_out_rate)


class StreamSenderPoolAV(StreamSenderPool):
    """StreamSenderPool for the whole link: the options of StreamSender -- ``rate``, ``audio="packets"`` with
    ``audio_books`` / ``audio_rate``, ``fec`` / ``audio_fec``, ``encoder`` -- with the same meaning and the same refusals.  Sessions
    are StreamSenderPool's (open / close / active / free / tokens).  Every session gets from ``step`` exactly what a
    ``StreamSender(batch=1)`` with the same options, fed the same samples, returns from ``push`` / ``finish``, byte for byte: the
    one item's values (a list of packets where the lockstep sender returns a list of one list).

    A tick IS StreamSenderPool's -- the class adds its constructor and nothing else; ``sender_pool_groups`` is unchanged, the
    options do not enter the launch parameters.  They only widen a group's rows, whose format the back end owns (_TxBack: bodies,
    book counts, audio bodies and counts, parity rows): still ONE device-to-host copy of all groups' rows, and
    _TxBack.frame_item per session with ITS chunk's sequence base."""

    _who = "StreamSenderPoolAV"

    def __init__(self, net, packet_tok=2, slots=64, books_use=None, rate=None, audio="packets", audio_books=None, audio_rate=None,
                 fec=None, audio_fec=None, encoder="window"):
        self._init_pool(net, packet_tok, slots, books_use, rate=rate, audio=audio, audio_books=audio_books, audio_rate=audio_rate,
                        fec=fec, audio_fec=audio_fec, encoder=encoder)
