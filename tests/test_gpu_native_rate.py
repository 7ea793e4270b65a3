"""-m gpu: the native-rate sender -- the rational streamed resampler against the whole-signal ``Resample`` (dense sessions and the
slots of a pool), and ``StreamSenderNative`` against compress_packets / compress_packets_av on the whole item resampled to 24 kHz
and crop_matched, with its options, and into the streaming receiver at 3 kHz.  Every comparison is an equality."""
import numpy as np
import pytest
import torch

from multimodal_vqvae_compression_audio_tactile_amd import bitstream, stream
from multimodal_vqvae_compression_audio_tactile_amd.packets import Fec, Rate

pytestmark = pytest.mark.gpu

_NETS, _REF, _SIG = {}, {}, {}
RATIOS = [(3000, 24000), (44100, 24000), (24000, 44100), (24000, 3000)]
TOKEN_HOLD = {(3000, 24000): 40, (44100, 24000): 4, (24000, 44100): 4, (24000, 3000): 40}     # blocks of one 320-sample token at 24 kHz
SR_A, SR_T = 44100, 3000
ITEMS = {"75tok": (44100, 3000), "ragged": (23270, 1583)}                  # native samples (audio, tactile); the second: 12664 at 24 kHz


def _net(dev, books=8, K=512, seed=7):
    """The b8_k512 model of golden_inputs.PE_CASES, as tests/test_gpu_sender.py builds it."""
    import golden_inputs as gi
    assert gi.PE_CASES["b8_k512"][:2] == (books, K) and gi.PE_CASES["b8_k512"][4] == seed
    if (books, K, seed) not in _NETS:
        from multimodal_vqvae_compression_audio_tactile_amd import build_proposed
        _NETS[(books, K, seed)] = build_proposed(gi.model_state(seed, books, K), rvq_books=books, rvq_embed=K, device=dev)
    return _NETS[(books, K, seed)]


# ----------------------------------------------------------------------------------------- 4. the kernel against Resample
def _state_want(x, S):
    """The last S samples of (zeros | x), oldest first."""
    B, n = x.shape
    return torch.cat([torch.zeros(B, S, device=x.device), x], dim=1)[:, n:]


@pytest.mark.parametrize("token_hold", [False, True])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("ratio", RATIOS)
def test_stream_resample_rational_equals_the_whole_signal(ratio, B, token_hold, dev):
    from multimodal_vqvae_compression_audio_tactile_amd import MvqError, Resample, StreamResampleRational, ops
    fi, fo = ratio
    whole = Resample(fi, fo).to(dev)
    orig, new, width = whole.orig, whole.new, whole.width
    hold = TOKEN_HOLD[ratio] if token_hold else None
    tok = TOKEN_HOLD[ratio] * orig                                         # input samples of one token
    ragged = 3 * orig + max(1, orig // 2)                                  # no multiple of orig (orig = 1: every count is one)
    pieces = [tok, 3 * tok, 16 * tok, 2 * orig, ragged]
    L = sum(pieces)
    x = torch.randn(B, 1, L, generator=torch.Generator().manual_seed(fi + fo + B)).to(dev)
    want = whole(x)
    assert want.shape == (B, 1, -(-new * L // orig))
    rs = StreamResampleRational(fi, fo, B, device=dev, hold=hold)
    h = rs.hold
    S = h * orig + width
    assert h == (TOKEN_HOLD[ratio] if token_hold else -(-width // orig)) and rs.state.shape == (B, S) and not rs.state.any()
    out, pos = [], 0
    for n in pieces[:-1]:
        y = rs.push(x[..., pos:pos + n])
        assert y.shape == (B, 1, stream.resample_stream_rational_out_len(pos, n, orig, new, width, hold))
        if token_hold and n % tok == 0:                                    # whole tokens in, whole tokens out, one token behind
            assert y.shape[-1] == TOKEN_HOLD[ratio] * new * (n // tok - (pos == 0))
        out.append(y)
        pos += n
        assert rs.consumed == pos and torch.equal(rs.state, _state_want(x[:, 0, :pos], S)), (n, pos)
    if orig > 1:                                                           # refused on the host: nothing moves
        before = rs.state.clone()
        with pytest.raises(MvqError, match="multiple"):
            rs.push(x[..., pos:pos + orig + 1])
        assert rs.consumed == pos and torch.equal(rs.state, before) and not rs.done
    out.append(rs.finish(x[..., pos:]))
    got = torch.cat(out, dim=-1)
    assert got.shape == want.shape and torch.equal(got, want)
    assert torch.equal(rs.state, _state_want(x[:, 0], S))
    with pytest.raises(MvqError, match="finished"):
        rs.push(x[..., :orig])
    with pytest.raises(MvqError, match="finished"):
        rs.finish()
    # a single-piece item goes to finish alone
    assert torch.equal(StreamResampleRational(fi, fo, B, device=dev, hold=hold).finish(x), want)
    # finish() without a piece flushes the tail alone
    rs = StreamResampleRational(fi, fo, B, device=dev, hold=hold)
    n_head = L - L % orig - 2 * orig
    head = rs.push(x[..., :n_head])
    tail = rs.finish()
    assert tail.shape[-1] > 0 and torch.equal(torch.cat([head, tail], dim=-1), whole(x[..., :n_head]))
    # the decimator's ratio at the decimator's lag: its outputs and its state, bit for bit
    if new == 1 and not token_hold:
        kern = rs.kernel
        st_r, st_d = ops.resample_stream_rational_state(orig, width, B, dev), ops.resample_stream_state(orig, width, B, dev)
        assert st_r.shape == st_d.shape
        pos = 0
        for i, n in enumerate(pieces):
            final = i == len(pieces) - 1
            y_r = ops.resample_stream_rational(x[:, 0, pos:pos + n], kern, st_r, pos, orig, new, width, final=final)
            y_d = ops.resample_stream(x[:, 0, pos:pos + n], kern, st_d, pos, orig, new, width, final=final)
            assert torch.equal(y_r, y_d) and torch.equal(st_r, st_d), i
            pos += n


def test_stream_resample_rational_refusals(dev):
    from multimodal_vqvae_compression_audio_tactile_amd import MvqError, StreamResampleRational, ops
    from multimodal_vqvae_compression_audio_tactile_amd.resample import sinc_resample_kernel
    with pytest.raises(MvqError, match="at least 7"):
        StreamResampleRational(3000, 24000, 1, device=dev, hold=6)
    with pytest.raises(MvqError, match="1024"):
        StreamResampleRational(44100, 24000, 1, device=dev, hold=7)
    kern, width, orig, new = sinc_resample_kernel(44100, 24000)
    kern = kern.to(dev)
    state = ops.resample_stream_rational_state(orig, width, 2, dev, hold=4)
    state.fill_(3.0)
    x = torch.ones(2, 1176, device=dev)
    for bad in (lambda: ops.resample_stream_rational(x, kern, state, 0, orig, new, width),                    # the state is hold = 4's
                lambda: ops.resample_stream_rational(x[:1], kern, state, 0, orig, new, width, hold=4),
                lambda: ops.resample_stream_rational(x, kern[:, :-1], state, 0, orig, new, width, hold=4),
                lambda: ops.resample_stream_rational(x, kern.cpu(), state, 0, orig, new, width, hold=4),
                lambda: ops.resample_stream_rational(x, kern, state.cpu(), 0, orig, new, width, hold=4),
                lambda: ops.resample_stream_rational(x, kern, state, 100, orig, new, width, hold=4),
                lambda: ops.resample_stream_rational(x[:, :1000], kern, state, 0, orig, new, width, hold=4)):
        with pytest.raises(MvqError):
            bad()
    assert bool((state == 3.0).all())


# ----------------------------------------------------------------------------------------------- 5. slots against dense
@pytest.mark.parametrize("ratio", [(44100, 24000), (3000, 24000)])
def test_resampler_rational_slots_equal_dense_sessions(ratio, dev):
    from multimodal_vqvae_compression_audio_tactile_amd import MvqError, ops
    from multimodal_vqvae_compression_audio_tactile_amd.resample import sinc_resample_kernel
    kern, width, orig, new = sinc_resample_kernel(*ratio)
    kern = kern.to(dev)
    hold = TOKEN_HOLD[ratio]
    tok = hold * orig
    S = hold * orig + width
    pool = torch.full((4, S), float("nan"), device=dev)                    # a session's first piece covers the state: nothing of it is read
    assert 2 * tok >= S
    sessions = {s: [ops.resample_stream_rational_state(orig, width, 1, dev, hold), 0] for s in (0, 2, 3)}   # dense state, consumed
    g = torch.Generator().manual_seed(ratio[0])
    # (group, n_new, final): 2 and 0 start, 3 starts, all three take a steady step (3 is at another position), then all end
    for group, n, final in (([2, 0], 2 * tok, False), ([3], 3 * tok, False), ([0, 2, 3], 5 * tok, False),
                            ([3, 0, 2], 2 * orig + max(1, orig // 2), True)):
        x = torch.randn(len(group), n, generator=g).to(dev)
        consumed = {sessions[s][1] for s in group}
        assert consumed == {0} or min(consumed) >= S                       # one launch class
        y = ops.resample_stream_rational_slots(x, kern, pool, group, max(consumed), orig, new, width, hold=hold, final=final)
        for i, s in enumerate(group):
            st, c = sessions[s]
            y1 = ops.resample_stream_rational(x[i:i + 1], kern, st, c, orig, new, width, hold=hold, final=final)
            assert y1.shape[1] > 0 and torch.equal(y[i:i + 1], y1), (group, s)
            assert torch.equal(pool[s:s + 1], st), (group, s)
            sessions[s][1] = c + n
        untouched = [s for s in range(4) if not sessions.get(s, [0, 0])[1]]
        assert 1 in untouched and bool(torch.isnan(pool[untouched]).all()), group
    keep = pool.clone()
    x = torch.zeros(2, tok, device=dev)
    for bad in ([0, 0], [0, 4], [-1, 2]):
        with pytest.raises(MvqError):
            ops.resample_stream_rational_slots(x, kern, pool, bad, 0, orig, new, width, hold=hold)
    with pytest.raises(MvqError, match="launch class"):
        ops.resample_stream_rational_slots(x, kern, pool, [0, 2], orig, orig, new, width, hold=hold)
    assert torch.equal(torch.nan_to_num(pool, nan=-7.0), torch.nan_to_num(keep, nan=-7.0))


# ------------------------------------------------------------------------------------------------- 6. the sender front end
def _signals(dev, B, na, nt, seed):
    from multimodal_vqvae_compression_audio_tactile_amd import synth
    if (B, na, nt, seed) not in _SIG:
        _SIG[(B, na, nt, seed)] = (synth.audio_segments(B, seed=seed, T=na, sr=SR_A).to(dev),
                                   synth.tactile_segments(B, seed=seed, T=nt, sr=SR_T).to(dev))
    return _SIG[(B, na, nt, seed)]


def _at_24k(dev, a, t):
    """The whole-item path's inputs: both signals through the whole-signal Resample, cropped to the shorter."""
    from multimodal_vqvae_compression_audio_tactile_amd import Resample, crop_match
    a24, t24 = crop_match(Resample(SR_A, 24000).to(dev)(a), Resample(SR_T, 24000).to(dev)(t))
    return a24.contiguous(), t24.contiguous()


def _case(dev, B, item):
    """compress_packets on the whole item at 24 kHz -- once per (B, item)."""
    if (B, item) not in _REF:
        na, nt = ITEMS[item]
        a, t = _signals(dev, B, na, nt, seed=na % 1000 + B)
        a24, t24 = _at_24k(dev, a, t)
        infos, pk, aud = _net(dev).compress_packets(a24, t24)
        codes = torch.from_numpy(np.stack([bitstream.unpack_indices(p)[0] for p in aud]))
        _REF[(B, item)] = (a, t, infos, pk, codes, a24.shape[-1])
    return _REF[(B, item)]


def _run_native(tx, a, t, pushes):
    """Feed a StreamSenderNative the pushes (tokens each), then finish with the rest -> (the steps' outputs, finish's whole tuple)."""
    ta, tt = tx.samples_per_token
    out, k = [], 0
    for m in pushes:
        out.append(tx.push(a[..., ta * k:ta * (k + m)], t[..., tt * k:tt * (k + m)]))
        k += m
    ra, rt = a[..., ta * k:], t[..., tt * k:]
    fin = tx.finish(ra if ra.shape[-1] else None, rt if rt.shape[-1] else None)
    return out, fin


def _cat(out, fin, k, n_info, b):
    """Element k of every push and of finish (whose StreamInfos sit behind its first two elements), item b, concatenated."""
    return sum((step[k][b] for step in out), []) + fin[k if k < 2 else k + n_info][b]


PUSHES = {"75tok": {"16": [16] * 4, "1": [1] * 75, "mixed": [3, 16, 7, 1, 16, 2, 16, 9]},
          "ragged": {"16": [16] * 2, "1": [1] * 39, "mixed": [3, 16, 7, 1, 5]}}


@pytest.mark.parametrize("item", sorted(ITEMS))
@pytest.mark.parametrize("B", [1, 2])
def test_sender_native_equals_compress_packets_on_the_resampled_item(B, item, dev):
    net = _net(dev)
    a, t, infos, pk, codes, L24 = _case(dev, B, item)
    na, nt = ITEMS[item]
    assert L24 == min(-(-80 * na // 147), 8 * nt) and (item != "ragged" or (L24 == 12664 == 8 * nt and L24 % 320))
    for name, pushes in PUSHES[item].items():
        tx = net.stream_sender_native(in_rates=(SR_A, SR_T), batch=B)
        assert tx.samples_per_token == (588, 40) and [rs.hold for rs in tx.rs] == [4, 40] and [rs.state.shape[1] for rs in tx.rs] == [600, 47]
        out, fin = _run_native(tx, a, t, pushes)
        assert len(fin) == 3 and fin[2] == infos[0] and tx.finished, name
        for b in range(B):
            assert _cat(out, fin, 0, 1, b) == pk[b], (name, b)                 # byte for byte, in order
        got = torch.cat([step[1] for step in out] + [fin[1]], dim=2)
        assert got.dtype == torch.int64 and torch.equal(got.cpu(), codes), name
        # the resamplers lag by one token: the inner session has seen m - 1 tokens after the first push, m more after each later one
        T = infos[0].T
        inner = ([pushes[0] - 1] if pushes[0] > 1 else []) + pushes[1:]
        sched = stream.sender_schedule(T, inner)[:len(inner)]
        emitted = [step[1].shape[2] for step in out]
        assert len(inner) == len(pushes) or emitted[0] == 0
        assert emitted[len(pushes) - len(inner):] == [min(16 * c1, T) - 16 * c0 if c1 > c0 else 0 for _, _, c0, c1, _ in sched], name


def test_sender_native_first_one_token_push_completes_nothing(dev):
    net = _net(dev)
    a, t = _case(dev, 1, "75tok")[:2]
    tx = net.stream_sender_native(batch=1)
    out = tx.push(a[..., :588], t[..., :40])
    assert out[0] == [[]] and out[1].shape == (1, 32, 0) and tx.tokens == 0
    assert [rs.consumed for rs in tx.rs] == [588, 40]
    assert torch.equal(tx.rs[0].state[:, -588:], a[:, 0, :588]) and torch.equal(tx.rs[1].state[:, -40:], t[:, 0, :40])   # the states moved
    tx.push(a[..., 588:588 * 4], t[..., 40:160])
    assert tx.tokens == 3
    with pytest.raises(ValueError, match="one m"):
        tx.push(a[..., :588 * 2], t[..., :40 * 3])
    with pytest.raises(ValueError, match="one m"):
        tx.push(a[..., :588 * 17], t[..., :40 * 17])
    with pytest.raises(ValueError, match="one m"):
        tx.push(a[..., :587], t[..., :40])
    assert tx.tokens == 3 and [rs.consumed for rs in tx.rs] == [588 * 4, 160]
    tx.finish()
    from multimodal_vqvae_compression_audio_tactile_amd import MvqError
    with pytest.raises(MvqError, match="after finish"):
        tx.push(a[..., :588], t[..., :40])
    with pytest.raises(ValueError, match="does not divide"):
        net.stream_sender_native(packet_tok=3)                                 # the inner session's refusal, its message
    with pytest.raises(ValueError, match="whole number"):
        net.stream_sender_native(in_rates=(44100, 2800))


# ------------------------------------------------------------------------------------------------------- 7. the crop rule
@pytest.mark.parametrize("tails", [(300, 18), (300, 25), (0, 3), (7, 0)])
def test_sender_native_crops_the_flushed_tails_to_the_shorter(tails, dev):
    """20 whole tokens, then final pieces whose 24 kHz lengths differ: (300, 18) -> 164 / 144 samples past the tokens (the tactile
    side is shorter), (300, 25) -> 164 / 200 (the audio side is), (0, 3) and (7, 0): one modality brings nothing to finish."""
    net = _net(dev)
    na, nt = 588 * 20 + tails[0], 40 * 20 + tails[1]
    a, t = _signals(dev, 1, na, nt, seed=na + nt)
    a24, t24 = _at_24k(dev, a, t)
    la, lt = -(-80 * na // 147), 8 * nt
    assert la != lt and a24.shape[-1] == t24.shape[-1] == min(la, lt)
    infos, pk, aud = net.compress_packets(a24, t24)
    out, fin = _run_native(net.stream_sender_native(batch=1), a, t, [16, 4])
    assert fin[2] == infos[0]
    assert _cat(out, fin, 0, 1, 0) == pk[0]
    got = torch.cat([step[1] for step in out] + [fin[1]], dim=2)
    assert torch.equal(got.cpu()[0], torch.from_numpy(bitstream.unpack_indices(aud[0])[0]))


# -------------------------------------------------------------------------------------------------- 8. options pass through
RATE, ARATE = Rate(min_books=2, tol2=0.84), Rate(min_books=2, tol2=0.5)
FEC, AFEC = Fec(4, 3), Fec(8, 4, 2)


def test_sender_native_with_rate_audio_packets_and_fec(dev):
    net = _net(dev)
    B = 2
    a, t = _case(dev, B, "ragged")[:2]
    opts = dict(rate=RATE, audio_rate=ARATE, fec=FEC, audio_fec=AFEC)
    infos, pk, ainfos, apk, par, apar = net.compress_packets_av(*_at_24k(dev, a, t), **opts)
    out, fin = _run_native(net.stream_sender_native(batch=B, audio="packets", **opts), a, t, PUSHES["ragged"]["mixed"])
    assert len(fin) == 6 and fin[2] == infos[0] and fin[3] == ainfos[0] and all(len(step) == 4 for step in out)
    for b in range(B):
        for k, want in enumerate((pk, apk, par, apar)):
            assert _cat(out, fin, k, 2, b) == want[b], (b, k)


def test_sender_native_with_the_stateful_encoder(dev):
    net = _net(dev)
    a, t, infos, pk, codes, _ = _case(dev, 2, "ragged")
    out, fin = _run_native(net.stream_sender_native(batch=2, encoder="stateful"), a, t, PUSHES["ragged"]["mixed"])
    assert fin[2] == infos[0]
    for b in range(2):
        assert _cat(out, fin, 0, 1, b) == pk[b], b
    assert torch.equal(torch.cat([step[1] for step in out] + [fin[1]], dim=2).cpu(), codes)


def test_sender_native_graph_replays_the_inner_steady_step(dev):
    net = _net(dev)
    na, nt = 588 * 97 + 100, 40 * 97 + 7                                       # six 16-token pushes bring 95 tokens at 24 kHz; the rest to finish
    a, t = _signals(dev, 1, na, nt, seed=97)
    eager, fin_e = _run_native(net.stream_sender_native(batch=1), a, t, [16] * 6)
    txg = net.stream_sender_native(batch=1, graph=True)
    graphed, fin_g = _run_native(txg, a, t, [16] * 6)
    assert txg.inner._g is not None and isinstance(txg.inner._g[0], torch.cuda.CUDAGraph)
    assert [len(step[0][0]) for step in eager] == [0, 8, 8, 8, 8, 8]            # chunk 0, then four steady steps: replays of the one graph
    for i, (e, g) in enumerate(zip(eager, graphed)):
        assert e[0] == g[0] and torch.equal(e[1], g[1]), i
    assert fin_e[0] == fin_g[0] and torch.equal(fin_e[1], fin_g[1]) and fin_e[2] == fin_g[2]
    infos, pk, aud = net.compress_packets(*_at_24k(dev, a, t))
    assert _cat(graphed, fin_g, 0, 1, 0) == pk[0] and fin_g[2] == infos[0]


# -------------------------------------------------------------------------------------------- 9. the whole link, native rates
def _seq(pkt):
    return int.from_bytes(bytes(pkt)[3:7], "little")


def test_sender_native_into_stream_receiver_at_3khz_equals_the_whole_item_link(dev):
    from multimodal_vqvae_compression_audio_tactile_amd import Resample
    net = _net(dev)
    B = 2
    a, t, infos, pk, codes, _ = _case(dev, B, "75tok")
    info = infos[0]
    out, fin = _run_native(net.stream_sender_native(batch=B), a, t, PUSHES["75tok"]["mixed"])
    sent = [_cat(out, fin, 0, 1, b) for b in range(B)]
    sent_codes = torch.cat([step[1] for step in out] + [fin[1]], dim=2)
    rng = np.random.default_rng(44100)
    keep = rng.random((B, info.P)) >= 0.3                                      # the seeded loss pattern: three packets in ten are lost
    assert not keep.all() and keep.any()
    rx = [[p for p in sent[b] if keep[b, _seq(p)]] for b in range(B)]
    aud = [bitstream.pack_indices(sent_codes[b].cpu().numpy(), 1024) for b in range(B)]
    want = Resample(24000, 3000).to(dev)(net.decompress_packets(infos, rx, aud)[0])
    rxr = net.stream_receiver(512, 8, batch=B, out_rate=3000)
    ys, T, per = [], info.T, 16 // info.packet_tok
    for c in range(T // 16):
        mine = [[p for p in item if c * per <= _seq(p) < (c + 1) * per] for item in rx]
        ys.append(rxr.push(mine, sent_codes[..., 16 * c:16 * c + 16]).clone())
    tail = [[p for p in item if _seq(p) >= (T // 16) * per] for item in rx]
    ys.append(rxr.finish(tail, sent_codes[..., T - T % 16:]) if T % 16 else rxr.finish())
    got = torch.cat(ys, dim=-1)
    assert got.shape == want.shape and torch.equal(got, want)
