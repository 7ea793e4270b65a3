"""CPU: the receiver pool's host logic -- the grouping of a tick's sessions and its plans against
StreamReceiver._plan and ops.resample_stream_out_len, the slot allocator, the new entry points' argument checks (null pointers:
refused before any device access), the slot-list checks of the ops wrappers, and the atomic tick."""
import numpy as np
import pytest
import torch

from multimodal_vqvae_compression_audio_tactile_amd import MvqError, packets, stream
from multimodal_vqvae_compression_audio_tactile_amd.packets import StreamInfo


@pytest.fixture(scope="module")
def cpu_net():
    from multimodal_vqvae_compression_audio_tactile_amd import build_proposed
    return build_proposed(None, rvq_books=2, rvq_embed=128, device="cpu")


# ----------------------------------------------------------------------------------------------------------- 1. grouping
def _sessions():
    """sid -> (tokens_before, n, last): pushes at every phase, finishers of n in {0, 5, 15} at every phase."""
    out, sid = {}, 0
    for before in (0, 16, 32, 48, 64):
        for n, last in ((16, False), (0, True), (5, True), (15, True)):
            out[sid] = (before, n, last)
            sid += 1
    return out


def test_pool_groups_keys_and_plans(cpu_net):
    from multimodal_vqvae_compression_audio_tactile_amd import ops
    sess = _sessions()
    groups = stream.pool_groups([(sid,) + v for sid, v in sess.items()])
    assert [g.key for g in groups] == sorted({(min(b, 32), n, last) for b, n, last in sess.values()})
    assert len(groups) == 12                                         # 3 phases x (push, finish 0 / 5 / 15)
    assert sorted(s for g in groups for s in g.sids) == sorted(sess)
    for g in groups:
        assert list(g.sids) == sorted(g.sids)                        # reproducible order
    by_sid = {s: g for g in groups for s in g.sids}
    # 32, 48 and 64 tokens share a group, 0 and 16 have their own
    for n, last in ((16, False), (0, True), (5, True), (15, True)):
        sids = {b: s for s, v in sess.items() for b in (v[0],) if v[1:] == (n, last)}
        assert by_sid[sids[32]] is by_sid[sids[48]] is by_sid[sids[64]]
        assert len({id(by_sid[sids[b]]) for b in (0, 16, 32)}) == 3
    # every member's own plan, as the solo session computes it, is the group's
    rx = cpu_net.stream_receiver(128, 2)
    for sid, (before, n, last) in sess.items():
        g = by_sid[sid]
        rx.tokens, rx.h = before, min(before, 20)
        assert rx._plan(n, last) == g.plan, (before, n, last)
        consumed = 320 * max(0, before - 10)                         # what the session has emitted: its resampler's `consumed`
        assert g.plan[3] - g.plan[2] == (max(0, 320 * (before + n) - 8) if last else 320 * max(0, before + n - 10)) - consumed
        assert ops.resample_stream_out_len(consumed, g.plan[3] - g.plan[2], 8, 49, final=last) == g.n_out
        assert ops.resample_stream_out_len(g.consumed, g.plan[3] - g.plan[2], 8, 49, final=last) == g.n_out
        # the launch class: base and lead of mvq_resample_stream_f32 from the member's consumed and from the group's
        assert (max(0, 56 - consumed), max(0, 105 - consumed)) == (max(0, 56 - g.consumed), max(0, 105 - g.consumed))
    steady = by_sid[[s for s, v in sess.items() if v == (48, 16, False)][0]]
    assert steady.key == (32, 16, False) and steady.plan == (20, 20, 3200, 8320) and (steady.consumed, steady.n_out) == (7040, 640)
    assert by_sid[[s for s, v in sess.items() if v == (0, 0, True)][0]].plan == (0, 0, 0, 0)
    assert stream.pool_groups([]) == []
    for bad in ((0, 8, 16, False), (0, 0, 15, False), (0, 0, 16, True), (0, -16, 16, False), (0, 0, -1, True)):
        with pytest.raises(ValueError):
            stream.pool_groups([bad])
    with pytest.raises(ValueError, match="twice"):
        stream.pool_groups([(3, 0, 16, False), (3, 16, 16, False)])


def test_resampler_constants_are_the_filter_design():
    from multimodal_vqvae_compression_audio_tactile_amd.resample import sinc_resample_kernel
    _, width, orig, new = sinc_resample_kernel(24000, 3000)
    assert (orig, width, new) == (stream.RS_ORIG, stream.RS_WIDTH, 1)


# ---------------------------------------------------------------------------------------------------- 2. constructor, slots
def test_pool_constructor_refusals(cpu_net):
    from multimodal_vqvae_compression_audio_tactile_amd import ProposedEval, StreamReceiverPool, ops
    assert StreamReceiverPool is stream.StreamReceiverPool and callable(ProposedEval.stream_receiver_pool)
    net = cpu_net
    for ptok in (3, 5, 32, 0):
        with pytest.raises(ValueError, match="does not divide"):
            net.stream_receiver_pool(128, 2, packet_tok=ptok)
    with pytest.raises(ValueError, match="plc"):
        net.stream_receiver_pool(128, 2, conceal="plc")
    with pytest.raises(ValueError, match="conceal"):
        net.stream_receiver_pool(128, 2, conceal="interpolate")
    with pytest.raises(ValueError, match="K = 512"):
        net.stream_receiver_pool(512, 2)
    with pytest.raises(ValueError, match="nb = 3"):
        net.stream_receiver_pool(128, 3)
    with pytest.raises(ValueError, match="out_rate"):
        net.stream_receiver_pool(128, 2, out_rate=8000)
    with pytest.raises(ValueError, match="slots"):
        net.stream_receiver_pool(128, 2, slots=0)
    assert ops.get_arith() == "f32"
    ops.set_arith("bf16x6")
    try:
        with pytest.raises(ValueError, match="arithmetic"):
            net.stream_receiver_pool(128, 2)
    finally:
        ops.set_arith("f32")
    pool = net.stream_receiver_pool(128, 2, slots=3, out_rate=3000)
    assert pool.carry.shape == (3, 1024) and pool.hist.shape == (3, 1024, 20) and pool.rs_state.shape == (3, 105)
    assert net.stream_receiver_pool(128, 2, slots=3).rs_state is None


def test_slot_allocator(cpu_net):
    pool = cpu_net.stream_receiver_pool(128, 2, slots=3)
    assert (pool.active, pool.free) == ((), 3)
    a, b, c = pool.open(), pool.open(), pool.open()
    assert len({a, b, c}) == 3 and pool.active == (a, b, c) and pool.free == 0
    assert [pool._sess[s][0] for s in (a, b, c)] == [0, 1, 2]
    with pytest.raises(MvqError, match="all 3 slots"):
        pool.open()
    assert pool.active == (a, b, c)
    # close frees the slot; the next session takes it, reset, under a sid of its own
    pool.carry[1].fill_(7.0)
    pool.close(b)
    assert pool.active == (a, c) and pool.free == 1
    with pytest.raises(MvqError, match="no open session"):
        pool.close(b)
    with pytest.raises(MvqError, match="no open session"):
        pool.tokens(b)
    d = pool.open()
    assert d not in (a, b, c) and pool._sess[d][0] == 1 and not pool.carry[1].any() and (pool.tokens(d), pool.late(d)) == (0, 0)
    # a session that finishes without a token runs nothing on the device and frees its slot: reuse after finish
    pool._sess[a][2] = 4
    out = pool.step({}, {a: None})
    assert list(out) == [a] and out[a].shape == (1, 1, 0)
    assert pool.active == (c, d) and pool.free == 1
    e = pool.open()
    assert pool._sess[e][0] == 0 and pool.late(e) == 0
    with pytest.raises(MvqError, match="no open session"):
        pool.step({a: ([], torch.zeros(32, 16, dtype=torch.int64))})
    pool.close(c), pool.close(d), pool.close(e)
    assert (pool.active, pool.free) == ((), 3) and pool._free == [0, 1, 2]
    assert pool.step({}) == {} and pool.step({}, {}) == {}


# -------------------------------------------------------------------------------------------------------- 3. entry points
def test_pool_entry_points_check_their_arguments():
    from multimodal_vqvae_compression_audio_tactile_amd import _lib, ops
    for n in ("stream_window_slots", "resample_stream_slots", "stream_rows"):
        assert callable(getattr(ops, n, None)), n
    lib = _lib.lib()
    for n in ("mvq_stream_window_slots_f32", "mvq_resample_stream_slots_f32", "mvq_stream_rows_f32"):
        assert n in _lib.EXPORTS and hasattr(lib, n), n
    assert lib.mvq_abi_version() == 3
    # every refusal below comes before any device access (no GPU here; all pointers null)
    win = lambda G=1, S=4, h_in=16, n=16, h_out=20, cap=20, c=96: \
        lib.mvq_stream_window_slots_f32(None, None, G, S, h_in, None, n, None, h_out, cap, c, None)
    assert win(h_out=33, cap=40) == -1 and b"exceeds h_in + n" in lib.mvq_last_error()
    assert win(h_in=21, n=15) == -1 and win(h_out=21) == -1                     # past the capacity
    for neg in (dict(G=-1), dict(S=-1), dict(h_in=-1), dict(n=-1), dict(h_out=-1), dict(cap=-1), dict(c=-96)):
        assert win(**neg) == -1, neg
    assert win(G=5, S=4) == -1 and b"pool of 4 slots" in lib.mvq_last_error()   # more sessions than slots: a repeated one
    assert win(G=3000000, S=3000000, c=1024) == -1                              # rows beyond 2^31 - 1
    assert win() == -1 and b"null" in lib.mvq_last_error()
    assert win(G=0) == 0 and win(h_in=0, n=0, h_out=0) == 0 and win(c=0) == 0   # empty: 0 without a launch
    rs = lambda G=1, S=4, n_new=1920, consumed=0, final=0, len_out=233, orig=8, newf=1, width=49, ks=106: \
        lib.mvq_resample_stream_slots_f32(None, None, None, None, G, S, None, n_new, consumed, final, len_out, orig, newf, width, ks, None)
    assert rs(newf=3) == -2                                                     # not a pure decimation
    assert rs(n_new=1921) == -1 and b"multiple" in lib.mvq_last_error()
    assert rs(consumed=4) == -1 and rs(ks=105) == -1
    assert rs(len_out=240) == -1 and b"233" in lib.mvq_last_error()
    assert rs(consumed=56, len_out=240) == -1 and b"launch class" in lib.mvq_last_error()     # inside the 105-sample state
    assert rs(G=-1) == -1 and rs(S=-1) == -1 and rs(n_new=-8) == -1 and rs(consumed=-8) == -1
    assert rs(G=5) == -1 and b"pool of 4 slots" in lib.mvq_last_error()
    assert rs() == -1 and b"null" in lib.mvq_last_error()
    assert rs(G=0) == 0 and rs(G=0, S=0) == 0
    assert rs(G=0, n_new=5120, consumed=7040, len_out=640) == 0 and rs(G=0, n_new=5120, consumed=1920, len_out=640) == 0
    assert rs(G=0, n_new=1592, consumed=12160, final=1, len_out=206) == 0       # final: ceil(1592/8) + 7
    assert rs(G=0, n_new=8, len_out=0, width=520, ks=1048) == -2                # a state beyond 1024 samples
    rows = lambda G=1, S=4, c=1024, scatter=0: lib.mvq_stream_rows_f32(None, None, G, S, None, c, scatter, None)
    assert rows(G=-1) == -1 and rows(S=-1) == -1 and rows(c=-1) == -1
    assert rows(G=5) == -1 and b"pool of 4 slots" in lib.mvq_last_error()
    assert rows(G=3000000, S=3000000) == -1
    assert rows() == -1 and rows(scatter=1) == -1 and b"null" in lib.mvq_last_error()
    assert rows(G=0) == 0 and rows(c=0) == 0


def test_ops_refuse_a_bad_slot_list_before_any_upload():
    """On CPU tensors nothing can be uploaded or launched: the slot list is what is checked first."""
    from multimodal_vqvae_compression_audio_tactile_amd import ops
    carry, hist, state = torch.zeros(5, 96), torch.zeros(5, 96, 20), torch.zeros(5, 105)
    z, x, kern = torch.zeros(2, 96, 16), torch.zeros(2, 1920), torch.zeros(1, 106)
    calls = {
        "stream_rows": lambda s: ops.stream_rows(carry, s),
        "stream_rows (scatter)": lambda s: ops.stream_rows(carry, s, rows=torch.zeros(2, 96)),
        "stream_window_slots": lambda s: ops.stream_window_slots(hist, s, 16, z, 20),
        "resample_stream_slots": lambda s: ops.resample_stream_slots(x, kern, state, s, 0, 8, 1, 49),
    }
    for name, call in calls.items():
        with pytest.raises(MvqError, match="listed twice"):
            call([3, 3])
        with pytest.raises(MvqError, match=r"slot 5 outside the pool's \[0, 5\)"):
            call([0, 5])
        with pytest.raises(MvqError, match="slot -1 outside"):
            call([-1, 2])
        with pytest.raises(MvqError, match="host integers"):
            call(torch.tensor([0, 1]))
        with pytest.raises(MvqError, match="host integers"):
            call([0.0, 1.0])
        with pytest.raises(MvqError, match="HIP tensor"):                       # a good list: the next check is the device
            call([4, np.int64(0)])


# ----------------------------------------------------------------------------------------------------- 4. the atomic tick
def test_a_bad_session_leaves_every_session_as_it_was(cpu_net):
    """Host logic only: every raise below comes from the tick's first phase, on a CPU-resident model."""
    pool = cpu_net.stream_receiver_pool(128, 2, slots=4)
    a, b, c = pool.open(), pool.open(), pool.open()
    info = StreamInfo(128, 2, 48, 2)
    pk = packets.frame(packets.pack_bodies(np.random.default_rng(3).integers(0, 128, size=(2, 48)), info), info)
    codes = torch.zeros(32, 16, dtype=torch.int64)
    pool._sess[a][1], pool._sess[b][1] = 32, 16                      # a has decoded two chunks, b one, c none
    pool._sess[a][2] = 1
    before = {s: (pool.tokens(s), pool.late(s)) for s in (a, b, c)}
    assert before == {a: (32, 1), b: (16, 0), c: (0, 0)}
    good_a = (pk[16:24] + [pk[3], pk[15]], codes)                    # two stragglers: would count as late
    good_b = ([pk[8], pk[2]], codes.unsqueeze(0))                    # one
    bad = [
        ({a: good_a, b: good_b, c: ([pk[8]], codes)}, None, ValueError, "seq 8"),                  # c: a packet of its next chunk
        ({a: good_a, b: good_b, c: ([], codes[:, :15])}, None, ValueError, "15 audio tokens"),
        ({a: good_a, b: good_b, c: ([], codes.float())}, None, ValueError, "audio_codes must be int"),
        ({a: good_a, b: good_b, c: ([], codes[:31])}, None, ValueError, "31 audio code rows"),
        ({a: good_a, b: good_b, c: ([], torch.zeros(2, 32, 16, dtype=torch.int64))}, None, ValueError, "audio_codes must be int"),
        ({a: good_a, b: good_b, 99: ([], codes)}, None, MvqError, "no open session 99"),
        ({a: good_a, b: good_b}, {b: None}, ValueError, "both pushed and finished"),
        ({a: good_a, b: good_b}, {c: ([], codes)}, ValueError, "16 audio tokens for a chunk of 1..15"),
        ({a: good_a, b: good_b}, {c: ([pk[0]], codes[:, :1])}, ValueError, "ntok"),
        ({a: good_a, b: good_b, c: None}, None, ValueError, "a push needs"),
        ({a: good_a, b: good_b, c: (b"garbage", codes)}, None, ValueError, None),
    ]
    for pushes, finishes, exc, match in bad:
        with pytest.raises(exc, match=match):
            pool.step(pushes, finishes)
        assert {s: (pool.tokens(s), pool.late(s)) for s in (a, b, c)} == before
        assert pool.active == (a, b, c) and pool.free == 1
    assert not pool.carry.any() and not pool.hist.any()
    # the same inputs without the bad session pass the host phase: its gather counts the stragglers, per session
    work = pool._inputs({a: good_a, b: good_b}, {c: ([pk[0]], codes[:, :2])})
    assert {s: (w[0], w[1], w[4]) for s, w in work.items()} == {a: (16, False, 2), b: (16, False, 1), c: (2, True, 0)}
    assert work[a][2][1].tolist() == [2] * 8 and work[b][2][1].tolist() == [2] + [0] * 7 and work[c][2][1].tolist() == [2]
    assert {s: (pool.tokens(s), pool.late(s)) for s in (a, b, c)} == before
