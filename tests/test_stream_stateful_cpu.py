"""CPU: the stateful streaming decoder's host arithmetic and the fact it rests on, restated from oracle
pieces (tests/stream_stateful_oracle.py).

  * the stage plan tiles every stage's output once and in order, inside the range the edge-loss rule calls exact, and emits what
    stream.schedule emits;
  * it depends on tokens_before only through the pool's grouping key;
  * the library's mvq_decoder_stream_plan says the same, number for number;
  * the staged decode equals the one-shot decode bit for bit on the oracle, and no longer does with one tail a column short;
  * the refusals."""
import ctypes

import numpy as np
import pytest
import torch

import stream_oracle as so
import stream_stateful_oracle as sso
from multimodal_vqvae_compression_audio_tactile_amd import stream

_ONE_SHOT = {}


def _sessions():
    """Every T in 1..100 as full chunks plus a finish of 0..15 tokens."""
    return [(T, sso.session_steps(T)) for T in range(1, 101)]


# --------------------------------------------------------------------------------------------------------------- 1. plan
def test_geometry_and_tails():
    assert stream.DEC_STAGES == ((1, 0, 3), (8, 0, 43), (5, -1, 41), (4, 0, 41), (2, 0, 40), (1, 0, 3))
    loss = 0
    for s, off, l in stream.DEC_STAGES:                              # 3 -> 67 -> 376 -> 1545 -> 3130 -> 3133: the measured halo
        loss = loss * s + l
    assert loss == 3133 == stream.DEC_HALO_SAMPLES[0] + 1
    assert stream.dec_stage_min_tails() == (6, 11, 17, 21, 40, 65) and stream.DEC_STAGE_TAILS == (8, 12, 20, 24, 40, 68)
    steady = stream.decoder_stage_plan(32, 16, False)
    assert [st.h_in + st.n_new for st in steady.stages] == [24, 28, 148, 664, 2600, 5188]      # every steady window a multiple of 4
    assert [st.n_new for st in steady.stages] == [16, 16, 128, 640, 2560, 5120] and (steady.e1 - steady.e0) == 5120


def test_plan_tiles_every_stage_and_emits_the_schedule():
    for T, steps in _sessions():
        assert len(steps) == T // 16 + 1 and sum(n for _, n, _ in steps) == T
        rows = sso.walk(steps)
        pos = [0] * 6
        for step, (before, n, last) in zip(rows, steps):
            for k, r in enumerate(step):
                assert 0 <= r["a"] <= r["b"] and r["h_out"] == (0 if last else min(stream.DEC_STAGE_TAILS[k], r["b"] - r["a"]))
                assert r["new0"] == pos[k] or r["new1"] == r["new0"], (T, before, k)            # in order, no gap, no overlap
                if r["new1"] > r["new0"]:
                    assert r["lo"] <= r["new0"] and r["new1"] <= r["hi"], (T, before, k, r)     # inside the exact range
                    pos[k] = r["new1"]
                if k + 1 < 6:                                                                    # what is handed on is the next stage's new input
                    assert step[k + 1]["b"] - step[k + 1]["a"] - step[k + 1]["h_in"] == r["new1"] - r["new0"]
                    assert r["new1"] == r["new0"] or step[k + 1]["b"] == r["new1"]
        # at the end every stage has handed on its whole output, and the emits are stream.schedule's
        t = T
        for k, (s, off, _) in enumerate(stream.DEC_STAGES):
            t = t * s + off
            assert pos[k] == t, (T, k)
        assert pos[5] == 320 * T - 8
        emits = [(step[5]["new0"], step[5]["new1"]) for step in rows]
        want = [(e0, e1) for _, _, e0, e1 in stream.schedule(T)]
        assert [e1 - e0 for e0, e1 in emits] == [e1 - e0 for e0, e1 in want]
        assert all(e == w for e, w in zip(emits, want) if w[1] > w[0])


def test_tokens_before_enters_only_through_the_pool_key():
    """pool_groups groups by (min(tokens_before, 32), n, last): sessions of one group must share the stage plan."""
    for n, last in [(16, False)] + [(m, True) for m in range(16)]:
        for before in range(0, 161, 16):
            key = min(before, 32)
            assert stream.decoder_stage_plan(before, n, last) == stream.decoder_stage_plan(key, n, last), (before, n, last)
        sessions = [(i, 16 * i, n, last) for i in range(8)]
        for g in stream.pool_groups(sessions):
            plans = {stream.decoder_stage_plan(16 * sid, n, last) for sid in g.sids}
            assert len(plans) == 1
            p = stream.decoder_stage_plan(g.key[0], n, last)
            assert p.e1 - p.e0 == g.plan[3] - g.plan[2]                                         # the window mode's emit length
    assert stream.decoder_stage_plan(16, 16) == stream.decoder_stage_plan(32, 16) != stream.decoder_stage_plan(0, 16)
    with pytest.raises(ValueError):
        stream.decoder_stage_plan(-1, 16)
    with pytest.raises(ValueError):
        stream.decoder_stage_plan(0, -1)


# ------------------------------------------------------------------------------------------------------- 2. the library
def test_library_plan_equals_python_plan():
    from multimodal_vqvae_compression_audio_tactile_amd import _lib, ops
    L = _lib.lib()
    dec = ops.Stack.decoder(1024, 1536, stream.DEC_RATES, 1, False)          # a description-only handle: no device call
    ns = L.mvq_decoder_stream_plan(dec.handle, 0, 0, 0, None, 0, None)
    assert ns == 6
    assert dec.decoder_stream_state_floats() == sum(c * t for c, t in zip((1024, 1536, 768, 384, 192, 96), stream.DEC_STAGE_TAILS)) == 65408
    cases = {st for _, steps in _sessions() for st in steps} | {(b, n, last) for b in (0, 1, 5, 7, 16, 21, 33) for n in (0, 1, 5, 16, 40)
                                                                 for last in (False, True)}
    for before, n, last in sorted(cases):
        stages, emit = dec.decoder_stream_plan(before, n, last)
        p = stream.decoder_stage_plan(before, n, last)
        assert tuple(s[:4] for s in stages) == tuple(tuple(s) for s in p.stages) and emit == (p.e0, p.e1), (before, n, last)
        assert tuple(s[4] for s in stages) == stream.DEC_STAGE_TAILS
    buf, emit = (ctypes.c_int32 * 30)(), (ctypes.c_int32 * 2)()
    assert L.mvq_decoder_stream_plan(dec.handle, 0, 16, 0, buf, 5, emit) == -1 and b"room for 5" in L.mvq_last_error()
    assert L.mvq_decoder_stream_plan(dec.handle, -1, 16, 0, buf, 6, emit) == -1 and L.mvq_decoder_stream_plan(dec.handle, 0, -1, 0, buf, 6, emit) == -1
    assert L.mvq_decoder_stream_plan(None, 0, 16, 0, buf, 6, emit) == -2
    enc = ops.Stack.encoder(64, (2, 4, 5, 8), 1024)
    assert L.mvq_decoder_stream_plan(enc.handle, 0, 16, 0, buf, 6, emit) == -2 and L.mvq_decoder_stream_state_floats(enc.handle) == 0
    padded = ops.Stack.decoder(1024, 1536, stream.DEC_RATES, 1, True)        # output_padding: the stage plan does not cover it
    assert L.mvq_decoder_stream_plan(padded.handle, 0, 16, 0, buf, 6, emit) == -2
    # the workspace query is host arithmetic too: the steady step needs less than the 36-token window it replaces
    assert 0 < L.mvq_decoder_stream_workspace_bytes(dec.handle, 1, 32, 16, 0) < L.mvq_decoder_workspace_bytes(dec.handle, 1, 36)
    assert L.mvq_decoder_stream_workspace_bytes(dec.handle, 0, 32, 16, 0) == 0 == L.mvq_decoder_stream_workspace_bytes(dec.handle, 1, -1, 16, 0)
    # the entry points refuse before any launch (no device here): no weights, null tensors
    assert L.mvq_decoder_stream_fwd_f32(dec.handle, None, None, 1, 1, None, 16, 0, 0, None, 1920, None, 0, None) == -1
    for fn in (L.mvq_stream_stage_window_f32, ):
        assert fn(None, 576, 12, None, 37, 1, 5, 16, None, 28, 1, 12, 12, 2, 48, None) == -1 and b"null" in L.mvq_last_error()
        assert fn(None, 576, 12, None, 37, 1, 22, 16, None, 28, 1, 12, 12, 2, 48, None) == -1 and b"outside the source rows" in L.mvq_last_error()
        assert fn(None, 576, 12, None, 37, 1, 5, 16, None, 28, 1, 12, 12, 0, 48, None) == 0                # an empty batch: nothing to do
    assert L.mvq_stream_stage_window_slots_f32(None, 576, None, 0, 4, 12, None, 37, 1, 5, 16, None, 28, 1, 12, 12, 48, None) == 0
    assert L.mvq_stream_stage_window_slots_f32(None, 576, None, 5, 4, 12, None, 37, 1, 5, 16, None, 28, 1, 12, 12, 48, None) == -1


# ------------------------------------------------------------------------------------------------ 3. staged decode, oracle
def _one_shot(orc, T):
    if T not in _ONE_SHOT:
        sd = so.dec_weights(7)
        z = so.latents(T, B=1)
        _ONE_SHOT[T] = (sd, z, orc.dac_decoder(sd, z, prefix="decoder."))
    return _ONE_SHOT[T]


@pytest.mark.parametrize("T", [11, 16, 37, 75])
def test_oracle_staged_decode_equals_one_shot(T, orc):
    sd, z, whole = _one_shot(orc, T)
    assert z.shape == (1, 1024, T) and whole.shape == (1, 1, 320 * T - 8)
    got = sso.staged_decode(orc, sd, z, sso.session_steps(T))
    assert got.shape == whole.shape and np.array_equal(got, whole)


def test_oracle_staged_decode_needs_every_tail_column(orc):
    """The last block's tail (40 columns, exactly the least) one column short: its first new output column misses a tap."""
    sd, z, whole = _one_shot(orc, 75)
    tails = list(stream.DEC_STAGE_TAILS)
    tails[4] -= 1
    assert tails[4] < stream.dec_stage_min_tails()[4]
    got = sso.staged_decode(orc, sd, z, sso.session_steps(75), tails=tuple(tails))
    assert got.shape == whole.shape and not np.array_equal(got, whole)


# ------------------------------------------------------------------------------------------------------------ 4. refusals
def test_stateful_refusals_come_before_any_launch():
    from multimodal_vqvae_compression_audio_tactile_amd import build_proposed, ops
    net = build_proposed(None, rvq_books=2, rvq_embed=128, device="cpu")
    with pytest.raises(ValueError, match="decoder must be 'window' or 'stateful'"):
        net.stream_receiver(128, 2, decoder="bogus")
    with pytest.raises(ValueError, match="decoder must be"):
        net.stream_receiver_pool(128, 2, slots=2, decoder="bogus")
    assert net.stream_receiver(128, 2).decoder == "window" and net.stream_receiver(128, 2).dec_state is None
    dec = ops.Stack.decoder(1024, 1536, stream.DEC_RATES, 1, False)
    S = dec.decoder_stream_state_floats()
    z = torch.zeros(1, 1024, 16)
    for bad in (torch.zeros(1, S - 1), torch.zeros(1, S + 4), torch.zeros(S), torch.zeros(1, S, dtype=torch.float64), None):
        with pytest.raises(ValueError, match="state must be"):
            dec.decoder_stream_fwd(bad, z, 0)
    with ops.arith("bf16x6"):
        with pytest.raises(ValueError, match="bf16x6"):
            dec.decoder_stream_fwd(torch.zeros(1, S), z, 0)
        with pytest.raises(ValueError, match="bf16x6"):
            net.stream_receiver(128, 2, decoder="stateful")
