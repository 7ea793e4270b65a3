"""CPU: the sender pool's host logic.

  * ``stream.sender_step``, the one function both sender classes take their arithmetic from, replayed push by push reproduces
    ``stream.sender_schedule`` entry by entry;
  * ``stream.sender_pool_groups``: which sessions of a tick share a launch sequence;
  * the new export, the C entry point's refusals (probed with null pointers: nothing can have been launched) and the host
    refusals of ``ops.stream_samples_slots``."""
import numpy as np
import pytest
import torch

from multimodal_vqvae_compression_audio_tactile_amd import stream

HOP = 320


# ---------------------------------------------------------------------------------------------------- 1. the step function
def _patterns(T):
    r = np.random.default_rng(T)
    mixed, used = [], 0
    while True:
        m = int(r.integers(1, 17))
        if used + m > T:
            break
        mixed.append(m)
        used += m
    return {"all16": [16] * (T // 16), "all1": [1] * T, "mixed": mixed}


def test_sender_step_replayed_reproduces_the_schedule():
    for T in range(1, 101):
        for name, pushes in _patterns(T).items():
            want = stream.sender_schedule(T, pushes)
            fill = start = chunk = 0
            got = []
            for i in range(len(pushes) + 1):
                last = i == len(pushes)
                n = HOP * (T - sum(pushes)) if last else HOP * pushes[i]
                st = stream.sender_step(fill, start, chunk, n, last)
                assert isinstance(st, stream.SenderStep)
                if st.emit:
                    assert st.w % HOP == 0 and st.drop % HOP == 0 and 0 <= st.lo < st.hi <= st.w // HOP
                    assert 16 * chunk == start + st.lo                                 # the first emitted token is the chunk's
                    assert st.w <= fill + n and st.drop <= fill + n and fill + n - st.drop == st.fill <= 48 * HOP
                    if not last:
                        assert st.hi - st.lo == 16 and (st.w // HOP, st.lo) == ((24, 0) if chunk == 0 else (32, 8))
                    got.append((start, start + st.w // HOP, chunk, st.chunk, st.fill // HOP))
                else:
                    assert (st.w, st.drop, st.start, st.chunk) == (0, 0, start, chunk)
                    got.append((start, start, chunk, chunk, st.fill // HOP))
                fill, start, chunk = st.fill, st.start, st.chunk
            assert got == want, (T, name)
    # finish with a ragged tail, and an item shorter than a token
    st = stream.sender_step(24 * HOP, 24, 2, 16 * HOP - 137, last=True)                # 40 tokens less 137 samples: 39 tokens
    assert st == stream.SenderStep(True, 40 * HOP - 137, 40 * HOP - 137, 8, 39, 0, 24, 4)
    assert stream.sender_step(0, 0, 0, 100, last=True) == stream.SenderStep(False, 0, 0, 0, 0, 0, 0, 0)
    assert stream.sender_step(0, 0, 0, 0, last=True).emit is False
    for bad in ((0, 0, 0, 100), (0, 0, 0, 0), (0, 0, 0, 17 * HOP), (-HOP, 0, 0, HOP), (100, 0, 0, HOP), (0, -1, 0, HOP), (0, 0, -1, HOP)):
        with pytest.raises(ValueError):
            stream.sender_step(*bad)


# ------------------------------------------------------------------------------------------------------------ 2. groups
def test_sender_pool_groups_keys_and_order():
    H = HOP
    sessions = [
        # (sid, fill, start, chunk, n, last)
        (9, 0, 0, 0, 16 * H, False),            # append: 16 tokens in hand
        (4, 23 * H, 0, 0, 1 * H, False),        # chunk 0: the 24th token arrives
        (2, 16 * H, 0, 0, 16 * H, False),       # chunk 0, another fill and push
        (7, 16 * H, 8, 1, 16 * H, False),       # steady, 16 held
        (1, 24 * H, 24, 2, 16 * H, False),      # steady, 24 held, a later chunk
        (5, 31 * H, 40, 3, 1 * H, False),       # steady, a 1-token push
        (3, 10 * H, 8, 1, 2 * H, False),        # append with a start of 8
        (8, 24 * H, 24, 2, 5 * H, True),        # finisher: 29 tokens, lo 8
        (6, 20 * H, 8, 1, 9 * H, True),         # finisher: the same fill + n and lo -> shares
        (10, 20 * H, 8, 1, 9 * H - 1, True),    # finisher: one sample less -> alone
        (11, 29 * H, 0, 0, 0, True),            # finisher: the same fill + n, but lo = 0 -> alone
        (12, 0, 0, 0, 100, True),               # finisher without a token: no device work, in no group
    ]
    groups = stream.sender_pool_groups(sessions)
    assert [g.key for g in groups] == [("append",), ("emit", 0), ("emit", 1), ("finish", 29 * H - 1, 8), ("finish", 29 * H, 0),
                                       ("finish", 29 * H, 8)]
    assert [g.sids for g in groups] == [(3, 9), (2, 4), (1, 5, 7), (10,), (11,), (6, 8)]             # sids ascending inside a group
    assert [(g.w, g.lo, g.hi) for g in groups] == [(0, 0, 0), (24 * H, 0, 16), (32 * H, 8, 24), (29 * H - 1, 8, stream.enc_tokens(29 * H - 1)), (29 * H, 0, 29),
                                                   (29 * H, 8, 29)]
    by_sid = {sid: st for g in groups for sid, st in zip(g.sids, g.steps)}
    assert 12 not in by_sid and len(by_sid) == 11
    for sid, fill, start, chunk, n, last in sessions[:-1]:
        assert by_sid[sid] == stream.sender_step(fill, start, chunk, n, last)
    # two sessions of different fill (and n, and drop) in one steady group; chunk 0 and steady never share
    steady = groups[2]
    assert {s.fill for s in steady.steps} == {24 * H, 16 * H} and len({(st.drop, st.w) for st in steady.steps}) == 1
    assert len({sessions[[s[0] for s in sessions].index(sid)][1] for sid in steady.sids}) == 3        # fills 16, 24 and 31 tokens
    assert not set(groups[1].sids) & set(groups[2].sids)
    assert stream.sender_pool_groups([]) == [] and stream.sender_pool_groups([sessions[-1]]) == []
    with pytest.raises(ValueError, match="listed twice"):
        stream.sender_pool_groups([sessions[0], sessions[0]])
    with pytest.raises(ValueError):
        stream.sender_pool_groups([(0, 0, 0, 0, 100, False)])


# ------------------------------------------------------------------------------------------------ 3. export and refusals
def test_sender_pool_entry_point_checks_its_arguments():
    from multimodal_vqvae_compression_audio_tactile_amd import ProposedEval, StreamSenderPool, _lib, ops
    assert StreamSenderPool is stream.StreamSenderPool and callable(ProposedEval.stream_sender_pool)
    assert callable(getattr(ops, "stream_samples_slots", None))
    lib = _lib.lib()
    assert "mvq_stream_samples_slots_f32" in _lib.EXPORTS and hasattr(lib, "mvq_stream_samples_slots_f32")
    assert lib.mvq_abi_version() == 3
    # refused before any device access (no GPU here): (buf, desc, n_group, n_slots, x_new, x_total, win, w, cap, stream)
    call = lambda G=2, S=4, x_total=640, w=0, cap=15360: lib.mvq_stream_samples_slots_f32(None, None, G, S, None, x_total, None, w, cap, None)
    for neg in (dict(G=-1), dict(S=-1), dict(x_total=-1), dict(w=-1), dict(cap=-1)):
        assert call(**neg) == -1 and b"negative" in lib.mvq_last_error(), neg
    assert call(cap=(1 << 24) + 1) == -1 and b"cap" in lib.mvq_last_error()
    assert call(G=5, S=4) == -1 and b"pool of 4" in lib.mvq_last_error()
    assert call() == -1 and b"null" in lib.mvq_last_error()                                # null pointers with a non-empty shape
    assert call(x_total=0, w=0) == -1 and call(x_total=0, w=10) == -1 and b"null" in lib.mvq_last_error()
    assert call(G=0) == 0 and call(G=0, S=0, x_total=0) == 0                               # empty: 0 without a launch


def test_ops_stream_samples_slots_refuses_on_the_host():
    """On CPU tensors nothing can have been launched: every one of these is refused by the host checks."""
    from multimodal_vqvae_compression_audio_tactile_amd import MvqError, ops
    buf = torch.zeros(4, 2, 15360)
    x = torch.zeros(2 * 320 + 2 * 640)
    good = [(3, 5120, 320, 0), (0, 0, 640, 0)]
    cases = {
        "repeated slot": ([(3, 5120, 320, 0), (3, 0, 640, 0)], x, 0),
        "slot out of range": ([(4, 5120, 320, 0), (0, 0, 640, 0)], x, 0),
        "negative slot": ([(-1, 5120, 320, 0), (0, 0, 640, 0)], x, 0),
        "negative fill": ([(3, -1, 320, 0), (0, 0, 640, 0)], x, 0),
        "negative n": ([(3, 5120, -320, 0)], x, 0),
        "negative drop": ([(3, 5120, 320, -1), (0, 0, 640, 0)], x, 0),
        "fill > cap": ([(3, 15361, 320, 0), (0, 0, 640, 0)], x, 0),
        "keep > cap": ([(3, 15360, 320, 319), (0, 0, 640, 0)], x, 0),
        "drop > fill + n": ([(3, 5120, 320, 5441), (0, 0, 640, 0)], x, 0),
        "w > fill + n": (good, x, 641),
        "negative w": (good, x, -1),
        "x_new too short": (good, x[:-1], 0),
        "x_new too long": (good, torch.zeros(x.numel() + 1), 0),
        "x_new not fp32": (good, x.double(), 0),
        "x_new not contiguous": (good, torch.zeros(2 * x.numel())[::2], 0),
        "a tensor for a session": ([torch.tensor([3, 5120, 320, 0])], x[:640], 0),
        "three integers": ([(3, 5120, 320)], x[:640], 0),
        "float entries": ([(3, 5120.0, 320, 0)], x[:640], 0),
    }
    for name, (sessions, xs, w) in cases.items():
        with pytest.raises(MvqError):
            ops.stream_samples_slots(buf, sessions, xs, w)
        pytest.raises(MvqError, ops.stream_samples_slots, buf, sessions, xs, w, torch.zeros(len(sessions), 5, dtype=torch.int32))
    with pytest.raises(MvqError, match=r"\[slots, 2, cap\]"):
        ops.stream_samples_slots(buf[:, 0], good, x, 0)
    with pytest.raises(MvqError):                                                          # a good call, but the pool is not on the device
        ops.stream_samples_slots(buf, good, x, 0)
    rows, x_total = ops.stream_samples_desc(good, 0, 15360)
    assert rows == [[3, 5120, 320, 0, 0], [0, 0, 640, 0, 640]] and x_total == 1920       # x_off: the exclusive prefix sum of 2n
    assert not buf.any()
