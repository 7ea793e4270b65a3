"""CPU restatement of the stateful streaming encoder, built only from oracle.conv1d, oracle.snake and
oracle._residual_unit.  Shared by tests/test_sender_stateful_cpu.py.

  * session_steps: the (samples_before, n, last) of a sender session, from stream.sender_step_stateful;
  * walk: the steps of a session in GLOBAL columns, reconstructed from the plan's local numbers -- per stage the window [a, b) of
    its input, the slice of its output it hands on, the range rule 2 calls exact;
  * staged_encode: every stage on [its tail | its new columns], the emitted pieces concatenated.  The tails are raw; the k3 stage's
    holds values that carry the final Snake already (oracle.snake on its producer's output), as on the device."""
import math

import numpy as np

from multimodal_vqvae_compression_audio_tactile_amd import stream

HOP = stream.HOP
RATES = stream.ENC_RATES


def session_steps(L, pushes):
    """The encoder steps of a sender session over L samples fed in ``pushes`` (tokens each) and a finish with the rest:
    (samples_before, n, last) of every step that runs the encoders, and per step the tokens [lo, hi) it must emit."""
    fill = start = chunk = pos = 0
    steps, emits = [], []
    for m in pushes:
        st = stream.sender_step_stateful(fill, start, chunk, HOP * m)
        pos += HOP * m
        if st.emit:
            assert st.drop == st.w and st.w <= fill + HOP * m
            steps.append((HOP * start, st.w, False))
            emits.append((start + st.lo, start + st.hi))
        fill, start, chunk = st.fill, st.start, st.chunk
    assert HOP * start + fill == pos
    st = stream.sender_step_stateful(fill, start, chunk, L - pos, last=True)
    if st.emit:
        assert st.w == st.drop == L - HOP * start
        steps.append((HOP * start, st.w, True))
        emits.append((start + st.lo, start + st.hi))
    return steps, emits


def walk(steps, tails=stream.ENC_STAGE_TAILS):
    """Per step and stage: dict(a, b, new0, new1, lo, hi, h_in, h_out) in global columns of the stage's input (a, b) and output
    (the rest): [new0, new1) is what the stage hands on, [lo, hi) what rule 2 calls exact for the window [a, b)."""
    have = [0] * len(stream.ENC_STAGES)
    out = []
    for before, n, last in steps:
        plan = stream.encoder_stage_plan(before, n, last, tails=tails)
        assert have[0] == before
        rows = []
        for k, ((s, ks, p, loss), st) in enumerate(zip(stream.ENC_STAGES, plan.stages)):
            a, b = have[k] - st.h_in, have[k] + st.n_new
            # J*s - p >= a + loss unless a == 0; J*s - p + ks <= b - loss, or the conv's own length when the edge is the signal's
            lo = 0 if a == 0 else -(-(a + loss + p) // s)
            hi = ((b + 2 * p - ks) // s + 1 if b > 0 and b + 2 * p - ks >= 0 else 0) if last else max(0, (b - loss + p - ks) // s + 1)
            nxt = plan.stages[k + 1] if k + 1 < len(plan.stages) else None
            n_out = nxt.n_new if nxt else plan.t1 - plan.t0
            new0 = a // s + (nxt.src_off if nxt else plan.off) if n_out else None
            rows.append(dict(a=a, b=b, s=s, new0=new0, new1=None if new0 is None else new0 + n_out, lo=lo, hi=hi, h_in=st.h_in, h_out=st.h_out))
            have[k] = b
        out.append((rows, (plan.t0, plan.t1)))
    return out


def _stage(orc, sd, k, win, P="encoder."):
    """Stage k of oracle.dac_encoder on a window (raw input; stage 5's input carries the final Snake already)."""
    if k == 0:
        w, b = orc._wn(sd, P + "block.0")
        return orc.conv1d(win, w, b, pad=3)
    if k <= len(RATES):
        s, p = RATES[k - 1], f"{P}block.{k}"
        h = win
        for j, dil in enumerate((1, 3, 9)):
            h = orc._residual_unit(sd, f"{p}.block.{j}", h, dil)
        w, b = orc._wn(sd, p + ".block.4")
        h = orc.conv1d(h, w, b, stride=s, pad=math.ceil(s / 2), alpha_in=sd[p + ".block.3.alpha"])
        if k == len(RATES):                                            # the producer of the k3 stage writes its output snaked
            h = orc.snake(h, sd[f"{P}block.{len(RATES) + 1}.alpha"])
        return h
    w, b = orc._wn(sd, f"{P}block.{len(RATES) + 2}")
    return orc.conv1d(win, w, b, pad=1)


def staged_encode(orc, sd, x, steps, tails=stream.ENC_STAGE_TAILS, align=True):
    """The encoder steps ``steps`` over the signal x[B, 1, L] -> the emitted latent columns concatenated."""
    tail = [None] * len(stream.ENC_STAGES)
    pieces, at = [], 0
    for before, n, last in steps:
        assert before == at
        plan = stream.encoder_stage_plan(before, n, last, tails=tails, align=align)
        src = np.ascontiguousarray(x[..., at:at + n])
        at += n
        for k, st in enumerate(plan.stages):
            new = src[..., st.src_off:st.src_off + st.n_new]
            if not align and new.shape[-1] < st.n_new:                 # off the stride grid the producer's window may end a column early
                new = np.concatenate([new, np.zeros(new.shape[:2] + (st.n_new - new.shape[-1],), np.float32)], axis=-1)
            assert new.shape[-1] == st.n_new and (st.h_in == 0 or tail[k].shape[-1] == st.h_in)     # the tail kept IS the tail read
            win = new if st.h_in == 0 else np.concatenate([tail[k], new], axis=-1)
            w = win.shape[-1]
            tail[k] = win[..., w - st.h_out:].copy()
            n_out = plan.stages[k + 1].n_new if k + 1 < len(plan.stages) else plan.t1 - plan.t0
            if w == 0 or n_out == 0:
                src = np.zeros(win.shape[:1] + (1, 0), np.float32)
                continue
            src = _stage(orc, sd, k, np.ascontiguousarray(win))
        pieces.append(src[..., plan.off:plan.off + plan.t1 - plan.t0])
    return np.concatenate(pieces, axis=-1)
