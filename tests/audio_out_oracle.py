"""The numpy restatement of the receiver's audio fade (packets.AudioFade is the definition, mvq_audio_fade_f32
the kernel): the whole-item form, written from the recurrences, and the PIECE form, which follows the streaming receiver's schedule
(16-token chunks, emission 10 tokens behind the newest token, a finish of 0..15 tokens) and keeps the state row the kernel keeps:
the saturated run lengths of the last 11 tokens received, the current run last.  tests/test_audio_out_cpu.py checks that the two
forms agree before any GPU test relies on either."""
import numpy as np

f32 = np.float32
HOP, TAIL, HALO, CHUNK = 320, 8, 10, 16
STATE = HALO + 1
FADES = [(0, 1), (1, 4), (2, 3)]
TOKENS = [1, 11, 16, 37, 75]
MASKS = ["all", "none", "first", "last", "alternating", "long_run", "border_run"]


def mask(name, T, H=1, F=4):
    """valid [T] uint8 (nonzero = some stage of the token arrived) of one of the seven patterns."""
    v = np.full(T, 3, np.uint8)
    if name == "all":
        pass
    elif name == "none":
        v[:] = 0
    elif name == "first":
        v[0] = 0
    elif name == "last":
        v[-1] = 0
    elif name == "alternating":
        v[1::2] = 0
    elif name == "long_run":                                  # one run longer than H + F, then tokens again when T allows it
        a = min(2, T - 1)
        v[a:a + H + F + 3] = 0
    elif name == "border_run":                                # a run that crosses the chunk border at token 16 (T permitting)
        v[max(0, min(T, CHUNK) - 3):CHUNK + 4] = 0
    else:
        raise KeyError(name)
    return v


def masks_for(B, T, H, F):
    """-> {name: valid [B, T]}: item b gets the pattern rolled by b tokens, so that a wrong batch stride shows."""
    return {m: np.stack([np.roll(mask(m, T, H, F), b) for b in range(B)]) for m in MASKS}


def runs(valid, H, F, r_prev=0):
    cap, r, out = H + F, int(r_prev), []
    for v in np.asarray(valid).reshape(-1):
        r = 0 if v else min(r + 1, cap)
        out.append(r)
    return np.asarray(out, np.int64)


def gain_of(r, H, F):
    r = np.asarray(r, np.int64)
    return np.where(r <= H, f32(1), (H + F - r).astype(f32) / f32(F)).astype(f32)


def _scale(y, g_prev, g, first_sample=0):
    """y [n] = the samples from ``first_sample`` of the token g[0] belongs to; g_prev = the gain of the token before g[0]."""
    s = np.arange(y.shape[0]) + first_sample
    t, j = s // HOP, s % HOP
    gg = np.concatenate([[g_prev], g]).astype(f32)
    g0, g1 = gg[t], gg[t + 1]
    w = (j + 1).astype(f32) / f32(HOP)
    d = (g1 - g0).astype(f32)
    m = (d * w).astype(f32)
    gain = (g0 + m).astype(f32)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(gain == 0, f32(0), (y * gain).astype(f32)).astype(f32), gain


def whole(y, valid, H, F):
    """y [B, 320*T - 8], valid [B, T] -> (faded, gain per sample), both float32 [B, 320*T - 8]."""
    y = np.asarray(y, f32)
    out, gains = np.empty_like(y), np.empty_like(y)
    for b in range(y.shape[0]):
        out[b], gains[b] = _scale(y[b], f32(1), gain_of(runs(valid[b], H, F), H, F))
    return out, gains


def steps(T):
    """The receiver's steps over T tokens: (tokens_before, n, last) -- one per whole chunk, then the finish of T % 16 tokens."""
    out = [(c * CHUNK, CHUNK, False) for c in range(T // CHUNK)]
    return out + [(T // CHUNK * CHUNK, T % CHUNK, True)]


def piece_range(before, n, last):
    """(tok0, first sample, end sample) of the piece the step emits."""
    tok0 = max(0, before - HALO)
    end = max(0, HOP * (before + n) - TAIL) if last else HOP * max(0, before + n - HALO)
    return tok0, HOP * tok0, end


def piece(y_piece, valid_new, state, H, F, before, n, last):
    """One step on one item: y_piece = the emitted samples, valid_new [n], state int [11] = r of the 11 tokens in front of the new
    ones (zeros at the start).  -> (faded piece, new state).  Only the state and the step's own valid are read."""
    state = np.zeros(STATE, np.int64) if before == 0 else np.asarray(state, np.int64)
    r_all = np.concatenate([state, runs(valid_new, H, F, r_prev=state[-1])])         # tokens before - 11 .. before + n - 1
    tok0, _, _ = piece_range(before, n, last)
    back = before - tok0                                                             # piece tokens in front of the new ones
    first = STATE - back                                                             # index of the piece's first token in r_all
    g = gain_of(r_all, H, F)
    out, _ = _scale(np.asarray(y_piece, f32), g[first - 1], g[first:])
    return out, r_all[-STATE:]


def pieces(y, valid, H, F):
    """The whole item through the schedule -> (concatenated faded pieces [B, 320*T - 8], the state rows after every step)."""
    y = np.asarray(y, f32)
    B, T = valid.shape
    state = np.zeros((B, STATE), np.int64)
    outs, states = [], []
    for before, n, last in steps(T):
        _, s0, s1 = piece_range(before, n, last)
        part = np.empty((B, s1 - s0), f32)
        for b in range(B):
            part[b], state[b] = piece(y[b, s0:s1], valid[b, before:before + n], state[b], H, F, before, n, last)
        outs.append(part)
        states.append(state.copy())
    return np.concatenate(outs, axis=1), states


def payload(B, T, seed):
    """A seeded waveform [B, 320*T - 8] in (-1, 1) with a few -0."""
    r = np.random.default_rng(seed)
    y = r.uniform(-1, 1, size=(B, max(0, HOP * T - TAIL))).astype(f32)
    y[:, ::97] = -0.0
    return y
