"""CPU: the stateful streaming encoder.

  * the stage plan tiles every stage's output once and in order, inside the range rule 2 calls exact, every window starts on a
    multiple of its stride, and the emitted tokens are stream.sender_schedule's;
  * it depends on samples_before only through the pool's grouping key;
  * the library's mvq_encoder_stream_plan says the same, number for number;
  * the staged encode equals oracle.dac_encoder bit for bit, and no longer does with one tail a column below the least or with a
    window start off the stride grid;
  * the refusals."""
import ctypes

import numpy as np
import pytest
import torch

import sender_oracle as sn
import sender_stateful_oracle as sso
from multimodal_vqvae_compression_audio_tactile_amd import stream
from test_sender_cpu import _patterns, _whole

HOP = stream.HOP


def _sessions():
    """Every T in 1..100 fed as all-16, all-1 and seeded mixed pushes, and the ragged length 320*40 - 137."""
    out = [(HOP * T, name, pushes) for T in range(1, 101) for name, pushes in _patterns(T).items()]
    return out + [(HOP * 40 - 137, "mixed", sn.split_pushes(HOP * 40 - 137, "mixed", seed=5)), (HOP * 40 - 137, "all16", [16, 16])]


# --------------------------------------------------------------------------------------------------------------- 1. plan
def test_geometry_and_tails():
    assert stream.ENC_STAGES == ((1, 7, 3, 0), (2, 4, 1, 39), (4, 8, 2, 39), (5, 10, 3, 39), (8, 16, 4, 39), (1, 3, 1, 0))
    lo = hi = 0                                                         # token 0 walked back to samples: the measured 8-token halo
    for s, ks, p, loss in reversed(stream.ENC_STAGES):
        lo, hi = lo * s - p - loss, hi * s - p + ks - 1 + loss
    assert (lo, hi) == (-2501, 2812)                                    # 7.82 tokens back, 7.79 past the token's own 320 samples
    assert -(-2501 // HOP) == -(-(2812 - (HOP - 1)) // HOP) == stream.ENC_HALO_TOK
    assert stream.enc_stage_min_tails() == (6, 81, 88, 90, 98, 2) and stream.ENC_STAGE_TAILS == (8, 84, 88, 92, 100, 4)
    assert [2 * 39 + ks - 1 for _, ks, _, _ in stream.ENC_STAGES[1:5]] == [81, 85, 87, 93]      # 77 + 2s; the rest is alignment slack
    # the least tails by brute force: over every count of input columns, what rule 1 and rule 2 need
    for (s, ks, p, loss), least in zip(stream.ENC_STAGES, stream.enc_stage_min_tails()):
        need = 0
        for have in range(1, 40 * s + 400):
            d = stream._enc_done(have, s, ks, p, loss)
            start = (d * s - p - loss) // s * s                        # the largest multiple of s the next window may start at
            need = max(need, have - max(start, 0))
        assert need == least, (s, need, least)
    first, steady = stream.encoder_stage_plan(0, 24 * HOP), stream.encoder_stage_plan(40 * HOP, 16 * HOP)
    assert (first.t0, first.t1) == (0, 16) and (steady.t0, steady.t1) == (32, 48)
    assert [st.n_new for st in steady.stages] == [5120, 5120, 2560, 640, 128, 16]
    assert [st.h_in + st.n_new for st in steady.stages] == [5128, 5203, 2646, 729, 228, 20]
    cols = sum(c * (st.h_in + st.n_new) for c, st in zip((1, 64, 128, 256, 512, 1024), steady.stages))
    once = sum(c * st.n_new for c, st in zip((1, 64, 128, 256, 512, 1024), steady.stages))
    assert 1.05 < cols / once < 1.25                                    # against 2.0 for the 32-token window


def test_plan_tiles_every_stage_and_emits_the_schedule():
    for L, name, pushes in _sessions():
        steps, emits = sso.session_steps(L, pushes)
        T = stream.enc_tokens(L)
        sched = [(16 * c0, min(16 * c1, T)) for _, _, c0, c1, _ in stream.sender_schedule(T, pushes) if c1 > c0]
        assert emits == sched, (L, name)                                # the host arithmetic emits sender_schedule's chunks ...
        rows = sso.walk(steps)
        assert [span for _, span in rows] == sched, (L, name)           # ... and so does the stage plan, token for token
        pos = [0] * 6
        for (step, _), (before, n, last) in zip(rows, steps):
            assert n <= (24 if before == 0 else 16) * HOP or last
            for k, r in enumerate(step):
                assert 0 <= r["a"] <= r["b"] and r["a"] % r["s"] == 0, (L, name, before, k)     # rule 1
                assert r["h_in"] <= stream.ENC_STAGE_TAILS[k] and r["h_out"] <= stream.ENC_STAGE_TAILS[k]
                if r["new0"] is not None:
                    assert r["new0"] == pos[k], (L, name, before, k)                            # in order, no gap, no overlap
                    assert r["lo"] <= r["new0"] and r["new1"] <= r["hi"], (L, name, before, k, r)   # rule 2
                    pos[k] = r["new1"]
                    if k + 1 < 6:
                        assert step[k + 1]["b"] == r["new1"]                                    # handed on = the next stage's new input
        t = L                                                           # at the end every stage has handed on its whole output
        for k, (s, ks, p, _) in enumerate(stream.ENC_STAGES):
            t = stream._enc_total(t, s, ks, p)
            assert pos[k] == t, (L, name, k)
        assert pos[5] == T


def test_samples_before_enters_only_through_the_pool_key():
    """sender_pool_groups(stateful=True) groups emitting pushes by min(chunk, 1) and finishers by (un-encoded samples, that class):
    the sessions of a group must share the stage plan."""
    first = stream.encoder_stage_plan(0, 24 * HOP)
    later = [stream.encoder_stage_plan(HOP * (16 * c + 8), 16 * HOP) for c in range(1, 12)]
    strip = lambda p: (p.stages, p.t1 - p.t0, p.off)                    # everything but the global token numbers
    assert len({strip(p) for p in later}) == 1 and strip(first) != strip(later[0])
    assert [(p.t0, p.t1) for p in later] == [(16 * c, 16 * c + 16) for c in range(1, 12)]
    for w in (0, 1, 137, 320, 2423, 5120, 12000, 39 * HOP):             # finishers: their un-encoded sample count and class
        plans = {strip(stream.encoder_stage_plan(HOP * (16 * c + 8), w, True)) for c in range(1, 12)}
        assert len(plans) == 1 and (w == 0 or strip(stream.encoder_stage_plan(0, w, True)) not in plans)
    # the groups themselves: sessions at chunks 0, 1, 2, 5 pushing 16 tokens onto what they hold, two finishers of one class
    held = lambda c: (8 * HOP, 0 if c == 0 else 16 * c + 8, c)          # (fill, start, chunk): 8 un-encoded tokens in hand
    sessions = [(i, *held(c), 16 * HOP, False) for i, c in enumerate((0, 1, 2, 5))] + [(4, *held(2), 100, True), (5, *held(7), 100, True),
                                                                                      (6, *held(0), 100, True)]
    groups = stream.sender_pool_groups(sessions, stateful=True)
    assert [(g.key, g.sids) for g in groups] == [(("emit", 0), (0,)), (("emit", 1), (1, 2, 3)), (("finish", 8 * HOP + 100, 0), (6,)),
                                                 (("finish", 8 * HOP + 100, 1), (4, 5))]
    for g in groups:
        last = g.key[0] == "finish"
        by_sid = {s[0]: s for s in sessions}
        plans = {strip(stream.encoder_stage_plan(HOP * by_sid[sid][2], g.w, last)) for sid in g.sids}
        assert len(plans) == 1 and next(iter(plans))[1] == g.hi - g.lo
    assert stream.sender_pool_groups(sessions[:4]) != groups[:2]        # the default grouping is the window mode's, untouched
    for bad in ((-1, 16), (0, -1), (0, stream.ENC_STREAM_MAX_N + 1)):
        with pytest.raises(ValueError):
            stream.encoder_stage_plan(*bad)


def test_stateful_step_feeds_each_sample_once():
    for L, name, pushes in _sessions():
        steps, _ = sso.session_steps(L, pushes)
        assert sum(n for _, n, _ in steps) == (L if steps else 0) and all(b == sum(n for _, n, _ in steps[:i]) for i, (b, _, _) in enumerate(steps))
        assert all(n == (24 if b == 0 else 16) * HOP for b, n, last in steps if not last), (L, name)
    st = stream.sender_step_stateful(8 * HOP, 24, 1, 16 * HOP)
    assert st == stream.SenderStep(True, 16 * HOP, 16 * HOP, -8, 8, 8 * HOP, 40, 2)
    assert stream.sender_step_stateful(0, 40, 2, 0, last=True) == stream.SenderStep(True, 0, 0, -8, 0, 0, 40, 3)   # the tails alone
    with pytest.raises(ValueError):
        stream.sender_step_stateful(0, 0, 0, 100)


# ------------------------------------------------------------------------------------------------------- 2. the library
def test_library_plan_equals_python_plan():
    from multimodal_vqvae_compression_audio_tactile_amd import _lib, ops
    L = _lib.lib()
    enc = ops.Stack.encoder(64, stream.ENC_RATES, 1024)                 # a description-only handle: no device call
    assert L.mvq_encoder_stream_plan(enc.handle, 0, 0, 0, None, 0, None) == 6
    assert enc.encoder_stream_state_floats() == sum(c * t for c, t in zip((1, 64, 128, 256, 512, 1024), stream.ENC_STAGE_TAILS)) == 95496
    cases = {st for Ls, _, pushes in _sessions()[::7] for st in sso.session_steps(Ls, pushes)[0]}
    cases |= {(b, n, last) for b in (0, 1, 5, 319, 320, 2501, 7680, 12663, 12800, 1 << 33) for n in (0, 1, 137, 320, 1600, 5120, 7680)
              for last in (False, True)}
    for before, n, last in sorted(cases):
        stages, emit = enc.encoder_stream_plan(before, n, last)
        p = stream.encoder_stage_plan(before, n, last)
        assert tuple(s[:4] for s in stages) == tuple(tuple(s) for s in p.stages) and emit == (p.t0, p.t1), (before, n, last)
        assert tuple(s[4] for s in stages) == stream.ENC_STAGE_TAILS
    buf, emit = (ctypes.c_int32 * 30)(), (ctypes.c_longlong * 2)()
    assert L.mvq_encoder_stream_plan(enc.handle, 0, 5120, 0, buf, 5, emit) == -1 and b"room for 5" in L.mvq_last_error()
    assert L.mvq_encoder_stream_plan(enc.handle, -1, 16, 0, buf, 6, emit) == -1 and L.mvq_encoder_stream_plan(enc.handle, 0, -1, 0, buf, 6, emit) == -1
    assert L.mvq_encoder_stream_plan(enc.handle, 0, stream.ENC_STREAM_MAX_N + 1, 0, buf, 6, emit) == -1
    assert L.mvq_encoder_stream_plan(None, 0, 16, 0, buf, 6, emit) == -2
    dec = ops.Stack.decoder(1024, 1536, stream.DEC_RATES, 1, False)
    assert L.mvq_encoder_stream_plan(dec.handle, 0, 16, 0, buf, 6, emit) == -2 and L.mvq_encoder_stream_state_floats(dec.handle) == 0
    # the workspace query is host arithmetic too: the steady step needs less than the 32-token window it replaces
    assert 0 < L.mvq_encoder_stream_workspace_bytes(enc.handle, 1, 40 * HOP, 16 * HOP, 0) < L.mvq_encoder_workspace_bytes(enc.handle, 1, 32 * HOP)
    assert L.mvq_encoder_stream_workspace_bytes(enc.handle, 0, 0, 5120, 0) == 0 == L.mvq_encoder_stream_workspace_bytes(enc.handle, 1, -1, 5120, 0)
    fn = L.mvq_stream_stage_window_snake_f32
    assert fn(None, 576, 12, None, 37, 5, 16, None, None, None, 28, 12, 12, 2, 48, None) == -1 and b"null" in L.mvq_last_error()
    assert fn(None, 576, 12, None, 37, 22, 16, None, None, None, 28, 12, 12, 2, 48, None) == -1 and b"outside the source rows" in L.mvq_last_error()
    assert fn(None, 576, 12, None, 37, 5, 16, None, None, None, 28, 12, 12, 0, 48, None) == 0              # an empty batch: nothing to do
    slots = L.mvq_stream_stage_window_snake_slots_f32
    assert slots(None, 576, None, 0, 4, 12, None, 37, 5, 16, None, None, None, 28, 12, 12, 48, None) == 0
    assert slots(None, 576, None, 5, 4, 12, None, 37, 5, 16, None, None, None, 28, 12, 12, 48, None) == -1


# ------------------------------------------------------------------------------------------------ 3. staged encode, oracle
@pytest.mark.parametrize("L", [320 * 11, 320 * 16, 320 * 37, 24000, 320 * 40 - 137])
def test_oracle_staged_encode_equals_one_shot(L, orc):
    sd, x, whole = _whole(orc, L)
    assert whole.shape == (1, 1024, stream.enc_tokens(L))
    steps, emits = sso.session_steps(L, sn.split_pushes(L, 16))
    got = sso.staged_encode(orc, sd, x, steps)
    assert got.shape == whole.shape and np.array_equal(got, whole)


def test_oracle_staged_encode_needs_every_tail_column_and_the_stride_grid(orc):
    # The least tails hold for ANY count of input columns; a sender session's steady counts do not reach every residue, so the
    # pieces here are 3003 + 2000 + 117 samples: after 3003 the second block (least 88 = its tail) has 1480 columns, its next
    # window must start at or below column 1392 and 87 columns reach back to 1393 only -- off the stride grid, so rule 1 moves
    # the start on to 1396, past the first new output's left-most input.
    sd, x, whole = _whole(orc, 5120)
    steps = [(0, 3003, False), (3003, 2000, False), (5003, 117, True)]
    assert np.array_equal(sso.staged_encode(orc, sd, x, steps), whole)
    tails = list(stream.ENC_STAGE_TAILS)
    tails[2] = stream.enc_stage_min_tails()[2] - 1
    short = sso.staged_encode(orc, sd, x, steps, tails=tuple(tails))
    assert short.shape == whole.shape and not np.array_equal(short, whole)
    # the plain tail min(cap, have): the strided convs' windows start off their stride grids
    sd, x, whole = _whole(orc, 24000)
    steps, _ = sso.session_steps(24000, sn.split_pushes(24000, 16))
    off_grid = sso.staged_encode(orc, sd, x, steps, align=False)
    assert off_grid.shape == whole.shape and not np.array_equal(off_grid, whole)


# ------------------------------------------------------------------------------------------------------------ 4. refusals
def test_stateful_refusals_come_before_any_launch():
    from multimodal_vqvae_compression_audio_tactile_amd import build_proposed, ops
    net = build_proposed(None, rvq_books=2, rvq_embed=128, device="cpu")
    with pytest.raises(ValueError, match="encoder must be 'window' or 'stateful'"):
        net.stream_sender(encoder="bogus")
    with pytest.raises(ValueError, match="encoder must be"):
        net.stream_sender_pool(slots=2, encoder="bogus")
    tx = net.stream_sender()
    assert tx.encoder == "window" and tx.enc_state is None and net.stream_sender_pool(slots=2).enc_state is None
    enc = ops.Stack.encoder(64, stream.ENC_RATES, 1024)
    S = enc.encoder_stream_state_floats()
    x = torch.zeros(1, 1, 5120)
    for bad in (torch.zeros(1, S - 1), torch.zeros(1, S + 4), torch.zeros(S), torch.zeros(1, S, dtype=torch.float64), None):
        with pytest.raises(ValueError, match="state must be"):
            enc.encoder_stream_fwd(bad, x, 0)
    with ops.arith("bf16x6"):
        with pytest.raises(ValueError, match="bf16x6"):
            enc.encoder_stream_fwd(torch.zeros(1, S), x, 0)
        with pytest.raises(ValueError, match="bf16x6"):
            net.stream_sender(encoder="stateful")
        with pytest.raises(ValueError, match="bf16x6"):
            net.stream_sender_pool(slots=2, encoder="stateful")
    # a wrong z_len and a short workspace are refused by the library before any launch (checked on the host: the z_len check
    # precedes every pointer check, the workspace check is plan_run's first step)
    from multimodal_vqvae_compression_audio_tactile_amd import _lib
    L = _lib.lib()
    fake = ctypes.addressof((ctypes.c_char * 64)())                    # non-null and never dereferenced: every call below is refused
    need = L.mvq_encoder_stream_workspace_bytes(enc.handle, 1, 0, 7680, 0)
    call = lambda z_len, ws: L.mvq_encoder_stream_fwd_f32(enc.handle, fake, None, 1, 1, fake, 7680, 0, 0, fake, z_len, fake, ws, None)
    assert call(15, need) == -1 and b"the step emits 16" in L.mvq_last_error()
    assert call(16, need - 1) == -1 and b"workspace too small" in L.mvq_last_error()
    assert call(16, need) == -1 and b"without weights" in L.mvq_last_error()      # a description-only handle: the last refusal
    assert L.mvq_encoder_stream_fwd_f32(enc.handle, None, None, 1, 1, None, 7680, 0, 0, None, 16, None, 0, None) == -1 and b"null" in L.mvq_last_error()
    assert L.mvq_encoder_stream_fwd_f32(enc.handle, fake, None, 2, 1, fake, 7680, 0, 0, fake, 16, fake, need, None) == -1   # 2 sessions, 1 state row
