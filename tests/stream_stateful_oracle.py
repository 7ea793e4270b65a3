"""CPU restatement of the stateful streaming decoder, built only from oracle.conv1d,
oracle.conv_transpose1d and oracle._residual_unit.  Shared by tests/test_stream_stateful_cpu.py.

  * walk: the steps of a session in GLOBAL columns, reconstructed from the plan's local numbers -- per stage the window [a, b) of its
    input, the slice of its output it hands on, the valid range by the edge-loss rule;
  * staged_decode: every stage on [its tail | its new columns], the emitted pieces concatenated.  The oracle applies a Snake at
    the consumer, so the tails here hold the values before it (the device's hold them after it: the same columns)."""
import math

import numpy as np

from multimodal_vqvae_compression_audio_tactile_amd import stream

RATES = stream.DEC_RATES


def session_steps(T, chunk=stream.CHUNK_TOK):
    """(tokens_before, n, last) of a session over T tokens: one push per full chunk, then the finish."""
    steps = [(b, chunk, False) for b in range(0, T - chunk + 1, chunk)]
    before = len(steps) * chunk
    return steps + [(before, T - before, True)]


def walk(steps, tails=stream.DEC_STAGE_TAILS):
    """Per step and stage: dict(a, b, new0, new1, lo, hi, out_len) in global columns of the stage's input (a, b) and output (the
    rest): [new0, new1) is what the stage hands on, [lo, hi) what the edge-loss rule calls exact.  And per step the emitted
    global sample range."""
    have = [0] * len(stream.DEC_STAGES)                   # input columns every stage has received
    out = []
    for before, n, last in steps:
        plan = stream.decoder_stage_plan(before, n, last, tails=tails)
        rows = []
        for k, ((s, off, loss), st) in enumerate(zip(stream.DEC_STAGES, plan.stages)):
            a = have[k] - st.h_in
            b = have[k] + st.n_new
            w = b - a
            out_len = w * s + off if w > 0 else 0
            lo = a * s + (0 if a == 0 else loss)
            hi = a * s + out_len - (0 if last else loss)
            nxt = plan.stages[k + 1] if k + 1 < len(plan.stages) else None
            new0 = a * s + (nxt.src_off if nxt else plan.e0)
            new1 = new0 + (nxt.n_new if nxt else plan.e1 - plan.e0)
            rows.append(dict(a=a, b=b, new0=new0, new1=new1, lo=lo, hi=hi, out_len=out_len, h_in=st.h_in, h_out=st.h_out))
            have[k] = b
        out.append(rows)
    return out


def _stage(orc, sd, k, win, P="decoder."):
    """Stage k of oracle.dac_decoder on a window."""
    if k == 0:
        w, b = orc._wn(sd, P + "model.0")
        return orc.conv1d(win, w, b, pad=3)
    if k <= len(RATES):
        s, p = RATES[k - 1], f"{P}model.{k}"
        w, b = orc._wn(sd, p + ".block.1")
        h = orc.conv_transpose1d(win, w, b, stride=s, pad=math.ceil(s / 2), alpha_in=sd[p + ".block.0.alpha"])
        for j, dil in enumerate((1, 3, 9)):
            h = orc._residual_unit(sd, f"{p}.block.{j + 2}", h, dil)
        return h
    n = len(RATES) + 1
    w, b = orc._wn(sd, f"{P}model.{n + 1}")
    return orc.conv1d(win, w, b, pad=3, alpha_in=sd[f"{P}model.{n}.alpha"], tanh=True)


def staged_decode(orc, sd, z, steps, tails=stream.DEC_STAGE_TAILS):
    """The session ``steps`` over the latents z[B, C, T] -> the emitted pieces concatenated."""
    tail = [None] * len(stream.DEC_STAGES)
    pieces, at = [], 0
    for before, n, last in steps:
        assert before == at
        plan = stream.decoder_stage_plan(before, n, last, tails=tails)
        src = np.ascontiguousarray(z[..., at:at + n])
        at += n
        for k, st in enumerate(plan.stages):
            new = src[..., st.src_off:st.src_off + st.n_new]
            assert new.shape[-1] == st.n_new
            win = new if st.h_in == 0 else np.concatenate([tail[k][..., :st.h_in], new], axis=-1)
            assert st.h_in == 0 or tail[k].shape[-1] >= st.h_in
            w = win.shape[-1]
            tail[k] = win[..., w - st.h_out:].copy()
            if w == 0:
                src = np.zeros(win.shape[:1] + (1, 0), np.float32)
                continue
            src = _stage(orc, sd, k, np.ascontiguousarray(win))
        pieces.append(src[..., plan.e0:plan.e1])
    return np.concatenate(pieces, axis=-1)
