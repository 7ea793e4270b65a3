"""-m gpu: the receiver's audio output at the playback rate.  Every comparison is an equality.

  1. the split form of the rational streamed resampler against the one-block form on a twin state, call by call, and the
     concatenation against the whole-signal ``Resample``;
  2. its slot form: guarded rows, a reversed group, each session against the dense form, an out-of-range slot;
  3. StreamReceiver(audio_out_rate=) eager and as a graph against Resample of the whole-item audio output;
  4. the whole-item calls;
  5. StreamReceiverPoolAV(audio_out_rate=) per session against a solo StreamReceiver(batch=1), a slot reused, two launch classes
     in a tick, a refused tick."""
import pytest
import torch

from multimodal_vqvae_compression_audio_tactile_amd import stream
from multimodal_vqvae_compression_audio_tactile_amd.packets import AudioFade, StreamInfo
from test_gpu_av import _channel, _signals

pytestmark = pytest.mark.gpu

_REF = {}
FADE = AudioFade(1, 4)
BOOKS, K, AUDIO = 2, 128, (1024, 32)
OPTS = dict(audio=AUDIO, audio_out=True, audio_fade=FADE, audio_conceal="hold")


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------ 1. split against block
RATIOS = [(24000, 44100), (24000, 48000), (24000, 22050), (24000, 12000), (44100, 24000)]
# pieces in tokens of the input rate (320 samples at 24 kHz, 588 at 44.1 kHz), then the final piece in samples less than a token
PATTERNS = {"a": ([6], 312), "b": ([1] * 6, 312), "c": ([2, 4], 0)}


def _twin_run(dev, ratio, B, pattern):
    """The pushes of ``pattern`` through both forms on twin states -> (concatenated outputs, the input that went in, Resample)."""
    from multimodal_vqvae_compression_audio_tactile_amd import Resample, ops
    fi, fo = ratio
    whole = Resample(fi, fo).to(dev)
    orig, new, width, kern = whole.orig, whole.new, whole.width, whole.kernel
    tok = 320 * fi // 24000 if fi == 24000 else 588
    assert tok % orig == 0
    toks, tail = PATTERNS[pattern]
    x = torch.randn(B, 7 * tok - 8, generator=torch.Generator().manual_seed(fi + fo)).to(dev)[:, :tok * sum(toks) + tail]
    st_s, st_b = ops.resample_stream_rational_state(orig, width, B, dev), ops.resample_stream_rational_state(orig, width, B, dev)
    S = st_s.shape[1]
    out, pos = [], 0
    for i, n in enumerate([tok * m for m in toks] + [tail]):
        final = i == len(toks)
        piece = x[:, pos:pos + n].contiguous()
        y_s = ops.resample_stream_rational(piece, kern, st_s, pos, orig, new, width, final=final, form="split")
        y_b = ops.resample_stream_rational(piece, kern, st_b, pos, orig, new, width, final=final, form="block")
        assert y_s.shape == y_b.shape == (B, stream.resample_stream_rational_out_len(pos, n, orig, new, width, None, final)), (i, n)
        assert torch.equal(y_s.view(torch.int32), y_b.view(torch.int32)), (ratio, pattern, i)
        assert torch.equal(st_s, st_b), (ratio, pattern, i)
        pos += n
        assert torch.equal(st_s, torch.cat([torch.zeros(B, S, device=dev), x[:, :pos]], dim=1)[:, pos:]), (ratio, pattern, i)
        out.append(y_s)
    return out, x, whole


@pytest.mark.parametrize("pattern", sorted(PATTERNS))
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("ratio", RATIOS)
def test_split_form_equals_the_block_form_and_the_whole_signal(ratio, B, pattern, dev):
    out, x, whole = _twin_run(dev, ratio, B, pattern)
    want = whole(x)
    got = torch.cat(out, dim=-1)
    assert got.shape == want.shape == (B, -(-whole.new * x.shape[1] // whole.orig)) and torch.equal(got, want)
    if ratio == (24000, 44100) and pattern == "a":
        assert out[0].shape[1] == 3381 == 23 * 147                        # a count no part count divides
    if ratio == (24000, 12000) and pattern == "b":
        assert 0 < out[-2].shape[1] <= 160 < 256                          # an n_out smaller than one part
    if pattern == "c":
        assert out[-1].shape[1] > 0                                       # the flush without new samples still writes the tail


def test_stream_resample_rational_takes_the_form(dev):
    from multimodal_vqvae_compression_audio_tactile_amd import Resample, StreamResampleRational
    x = torch.randn(2, 1, 2232, generator=torch.Generator().manual_seed(5)).to(dev)
    rs = StreamResampleRational(24000, 44100, 2, device=dev, form="split")
    got = torch.cat([rs.push(x[..., :1920]), rs.finish(x[..., 1920:])], dim=-1)
    assert rs.form == "split" and torch.equal(got, Resample(24000, 44100).to(dev)(x))


# ------------------------------------------------------------------------------------------------------------- 2. slots
@pytest.mark.parametrize("ratio", [(24000, 44100), (24000, 48000), (24000, 22050)])
def test_split_slot_form(ratio, dev):
    from multimodal_vqvae_compression_audio_tactile_amd import MvqError, Resample, _lib, ops
    whole = Resample(*ratio).to(dev)
    orig, new, width, kern = whole.orig, whole.new, whole.width, whole.kernel
    hold = -(-width // orig)
    S = hold * orig + width
    group = [2, 0]                                                          # item 0 is slot 2, item 1 slot 0
    pool = torch.full((4, S), float("nan"), device=dev)
    pool_b = pool.clone()
    for p in (pool, pool_b):
        p[group] = 0.0                                                      # what open() does
    dense = [ops.resample_stream_rational_state(orig, width, 1, dev) for _ in group]
    x = torch.randn(2, 2232, generator=torch.Generator().manual_seed(ratio[1])).to(dev)
    out, pos = [], 0
    for i, n in enumerate([320] * 6 + [312]):
        final = i == 6
        assert pos == 0 or pos >= S                                         # a launch class
        piece = x[:, pos:pos + n].contiguous()
        y = ops.resample_stream_rational_slots(piece, kern, pool, group, pos, orig, new, width, final=final, form="split")
        y_b = ops.resample_stream_rational_slots(piece, kern, pool_b, group, pos, orig, new, width, final=final, form="block")
        assert torch.equal(y.view(torch.int32), y_b.view(torch.int32)), i
        for g, s in enumerate(group):
            y1 = ops.resample_stream_rational(piece[g:g + 1], kern, dense[g], pos, orig, new, width, final=final, form="split")
            assert torch.equal(y[g:g + 1], y1) and torch.equal(pool[s:s + 1], dense[g]) and torch.equal(pool_b[s], pool[s]), (i, g)
        assert bool(torch.isnan(pool[[1, 3]]).all()), i                     # rows that no slot names keep their NaN bits
        assert torch.equal(pool[[1, 3]].view(torch.int32), pool_b[[1, 3]].view(torch.int32))
        out.append(y)
        pos += n
    assert torch.equal(torch.cat(out, dim=-1), whole(x))
    # the device copy of the list, when the caller uploaded it already
    pa, pb = pool.clone(), pool.clone()
    piece = x[:, :320].contiguous()
    ya = ops.resample_stream_rational_slots(piece, kern, pa, group, 2240, orig, new, width, form="split")
    yb = ops.resample_stream_rational_slots(piece, kern, pb, group, 2240, orig, new, width, form="split",
                                            slots_dev=torch.tensor(group, dtype=torch.int32, device=dev))
    assert torch.equal(ya, yb) and torch.equal(pa[group], pb[group])
    # an out-of-range slot: the wrapper refuses it on the host in both forms and nothing moves ...
    keep = pool.clone()
    for form in ("block", "split"):
        for bad in ([0, 4], [-1, 2], [0, 0]):
            with pytest.raises(MvqError):
                ops.resample_stream_rational_slots(piece, kern, pool, bad, 2240, orig, new, width, form=form)
    assert torch.equal(pool.view(torch.int32), keep.view(torch.int32))
    # ... and in a direct C call both kernels read a zero state for it and store none
    lib = _lib.lib()
    sd = torch.tensor([2, 7], dtype=torch.int32, device=dev)
    n_out = stream.resample_stream_rational_out_len(2240, 320, orig, new, width)
    res = {}
    for form, fn in (("block", lib.mvq_resample_stream_rational_slots_f32), ("split", lib.mvq_resample_stream_rational_split_slots_f32)):
        p, y = keep.clone(), torch.full((2, n_out), float("nan"), device=dev)
        rc = fn(piece.data_ptr(), kern.data_ptr(), p.data_ptr(), sd.data_ptr(), 2, 4, y.data_ptr(), 320, 2240, 0, n_out, orig, new, width,
                2 * width + orig, hold, _stream())
        assert rc == 0, lib.mvq_last_error()
        res[form] = (p, y)
        assert torch.equal(p[[0, 1, 3]].view(torch.int32), keep[[0, 1, 3]].view(torch.int32)) and not torch.equal(p[2], keep[2])
        zero = ops.resample_stream_rational_state(orig, width, 1, dev)      # the out-of-range session: the piece on a zero state
        assert torch.equal(y[1:2], ops.resample_stream_rational(piece[1:2], kern, zero, 2240, orig, new, width, form=form))
    assert torch.equal(res["block"][1], res["split"][1]) and torch.equal(res["block"][0][2], res["split"][0][2])


# --------------------------------------------------------------------------------------------------- 3. StreamReceiver
def _anet(dev):
    """2 books x K = 128 with the audio decoder attached (build_proposed(audio_decoder=True)) under seeded weights."""
    if "net" not in _REF:
        import golden_inputs as gi
        from multimodal_vqvae_compression_audio_tactile_amd import build_proposed
        net = build_proposed(gi.model_state(7, BOOKS, K), rvq_books=BOOKS, rvq_embed=K, device=dev, audio_decoder=True)
        sd = gi.model_state(23, BOOKS, K)
        net.audio_decoder.load_state_dict({k[len("T_DEC."):]: v for k, v in sd.items() if k.startswith("T_DEC.")}, strict=True)
        _REF["net"] = net
    return _REF["net"]


def _seq(p):
    return int.from_bytes(bytes(p)[3:7], "little")


def _item(dev, T, B=2):
    """B items of T tokens through compress_packets_av and a seeded lossy channel on both streams, and the whole-item outputs --
    computed once per (T, B)."""
    if ("item", T, B) not in _REF:
        net = _anet(dev)
        a, t = _signals(dev, B, 320 * T)
        infos, pk, ainfos, apk = net.compress_packets_av(a, t)
        info, ainfo = infos[0], ainfos[0]
        assert info == StreamInfo(K, BOOKS, T, 2) and ainfo == StreamInfo(1024, 32, T, 2)
        rx = [_channel(pk[b], info, 10 * b + T)[0] for b in range(B)]
        arx = [_channel(apk[b], ainfo, 10 * b + T + 3)[0] for b in range(B)]
        whole = net.decompress_packets_av([info] * B, rx, [ainfo] * B, arx, audio_conceal="hold", audio_out=True, audio_fade=FADE)
        assert whole[3].shape == (B, 1, 320 * T - 8)
        assert T < 37 or (bool(whole[1].any()) and bool(whole[2].any()))       # loss on both streams
        _REF[("item", T, B)] = dict(info=info, ainfo=ainfo, rx=rx, arx=arx, whole=whole, a=a, t=t)
    return _REF[("item", T, B)]


def _chunk(it, c, last, b=None):
    """What arrives of chunk c (``last``: everything from it on), per item of the batch or for item b alone."""
    ok = (lambda p: _seq(p) >= 8 * c) if last else (lambda p: 8 * c <= _seq(p) < 8 * c + 8)
    pick = lambda lists: [[p for p in lst if ok(p)] for lst in lists]
    tp, ap = pick(it["rx"]), pick(it["arx"])
    return (tp, ap) if b is None else (tp[b], ap[b])


def _run(dev, T, B=2, **kw):
    """A StreamReceiver over the item of T tokens -> [(y, y_audio)] call by call."""
    it = _item(dev, T, B)
    rx = _anet(dev).stream_receiver(K, BOOKS, batch=B, **OPTS, **kw)
    outs = []
    for c in range(T // 16):
        tp, ap = _chunk(it, c, False)
        outs.append(tuple(o.clone() for o in rx.push(tp, audio_packets=ap)))
    if T % 16:
        tp, ap = _chunk(it, T // 16, True)
        outs.append(rx.finish(tp, ap, tokens=T % 16))
    else:
        outs.append(rx.finish())
    return outs, rx


def _plain(dev, T, B=2, **kw):
    key = ("plain", T, B, tuple(sorted(kw.items())))
    if key not in _REF:
        _REF[key] = _run(dev, T, B, **kw)[0]
    return _REF[key]


def _want_audio(dev, T, rate, B=2):
    from multimodal_vqvae_compression_audio_tactile_amd import Resample
    key = ("want", T, rate, B)
    if key not in _REF:
        _REF[key] = Resample(24000, rate).to(dev)(_item(dev, T, B)["whole"][3])
    return _REF[key]


STREAM_CASES = [(37, r, g, {}) for r in (44100, 48000) for g in (False, True)] + \
               [(37, 44100, False, dict(out_rate=3000, decoder="stateful")),
                (53, 44100, True, {}),                                          # three pushes: the steady step is captured and replayed
                (5, 48000, False, {})]                                          # a finish only


@pytest.mark.parametrize("T,rate,graph,kw", STREAM_CASES)
def test_stream_receiver_audio_at_the_playback_rate(T, rate, graph, kw, dev):
    outs, rx = _run(dev, T, graph=graph, audio_out_rate=rate, **kw)
    plain = _plain(dev, T, graph=graph, **kw)
    want = _want_audio(dev, T, rate)
    orig, new = rx.ars_plan[:2]
    assert len(outs) == len(plain) == T // 16 + 1
    for j, ((y, ya), (y0, ya0)) in enumerate(zip(outs, plain)):
        assert y.shape == y0.shape and torch.equal(y, y0), j                    # the tactile pieces: the session at 24000
        assert ya.shape[:2] == (2, 1) and (j == len(outs) - 1 or ya.shape[-1] % new == 0), j
    got = torch.cat([o[1] for o in outs], dim=-1)
    assert got.shape == want.shape == (2, 1, -(-new * (320 * T - 8) // orig))
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert torch.equal(torch.cat([o[1] for o in plain], dim=-1), _item(dev, T)["whole"][3])
    if graph and T >= 48:
        assert rx._g is not None and isinstance(rx._g[0], torch.cuda.CUDAGraph)
    if kw:
        assert outs[0][0].shape[-1] < 1920 // 8 + 1 and rx.rs_state is not None  # the tactile output left at 3 kHz


def test_stream_receiver_empty_finish(dev):
    rx = _anet(dev).stream_receiver(K, BOOKS, batch=2, audio_out_rate=44100, **OPTS)
    keep = rx.ars_state.clone()
    y, ya = rx.finish()
    assert y.shape == ya.shape == (2, 1, 0) and torch.equal(rx.ars_state, keep)


# ------------------------------------------------------------------------------------------------------- 4. whole item
def test_whole_item_calls(dev):
    from multimodal_vqvae_compression_audio_tactile_amd import Resample
    net, it = _anet(dev), _item(dev, 37)
    args = ([it["info"]] * 2, it["rx"], [it["ainfo"]] * 2, it["arx"])
    kw = dict(audio_conceal="hold", audio_out=True, audio_fade=FADE)
    base = it["whole"]
    at_24 = net.decompress_packets_av(*args, audio_out_rate=24000, **kw)
    assert len(at_24) == 4 and all(torch.equal(g, w) for g, w in zip(at_24, base))
    want = _want_audio(dev, 37, 44100)
    got = net.decompress_packets_av(*args, audio_out_rate=44100, **kw)
    assert all(torch.equal(g, w) for g, w in zip(got[:3], base[:3]))            # the tactile output and both loss maps are unchanged
    assert got[3].shape == want.shape and torch.equal(got[3].view(torch.int32), want.view(torch.int32))
    _, codes, idx = net.encode_latents_with_indices(it["a"], it["t"])
    y0, ya0 = net.decode_av(codes, idx)
    y1, ya1 = net.decode_av(codes, idx, audio_out_rate=24000)
    y2, ya2 = net.decode_av(codes, idx, audio_out_rate=44100)
    assert torch.equal(y1, y0) and torch.equal(ya1, ya0) and torch.equal(y2, y0)
    assert torch.equal(ya2, Resample(24000, 44100).to(dev)(ya0)) and ya2.shape[-1] == -(-147 * (320 * 37 - 8) // 80)


# -------------------------------------------------------------------------------------------------------------- 5. pool
POOL_TOKENS, POOL_OPENS = (37, 16, 11), (0, 0, 2)      # session 1 ends at tick 1, session 2 takes its slot at tick 2


def test_pool_av_audio_at_the_playback_rate(dev):
    from multimodal_vqvae_compression_audio_tactile_amd import MvqError
    net = _anet(dev)
    kw = dict(audio_out_rate=44100, **OPTS)
    pool = stream.StreamReceiverPoolAV(net, K, BOOKS, slots=2, **kw)
    pool.ars_state.fill_(float("nan"))                                        # open() zeroes a session's row
    pool.a_hist.fill_(float("nan"))                                           # ... and a new session reads no history and no run length
    pool.fade_state.fill_(0x7FC00000)
    items = [_item(dev, T, 1) for T in POOL_TOKENS]
    sids, nxt, done, outs, classes, tick = {}, {}, set(), {k: [] for k in range(3)}, [], 0
    while len(done) < 3:
        for k, t0 in enumerate(POOL_OPENS):
            if t0 == tick:
                sids[k], nxt[k] = pool.open(), 0
        pushes, finishes, cls = {}, {}, set()
        for k, sid in sids.items():
            if k in done:
                continue
            T, c = POOL_TOKENS[k], nxt[k]
            cls.add(320 * max(0, 16 * c - 10))
            if 16 * (c + 1) <= T:
                pushes[sid] = _chunk(items[k], c, False, 0)
            elif T % 16:
                finishes[sid] = stream.PoolChunk(*_chunk(items[k], c, True, 0), tokens=T % 16)
            else:
                finishes[sid] = None
        if tick == 1:                                                         # a refused tick moves no state
            keep = pool.ars_state.clone()
            with pytest.raises(ValueError, match="both pushed and finished"):
                pool.step(pushes, {**finishes, next(iter(pushes)): None})
            with pytest.raises(MvqError, match="no open session"):
                pool.step({**pushes, 9999: next(iter(pushes.values()))}, finishes)
            torch.cuda.synchronize()
            assert torch.equal(pool.ars_state.view(torch.int32), keep.view(torch.int32))
        out = pool.step(pushes, finishes)
        classes.append(cls)
        for k, sid in sids.items():
            if sid in out:
                outs[k].append(out[sid])
            if sid in pushes:
                nxt[k] += 1
            elif sid in finishes:
                done.add(k)
        tick += 1
    assert pool.active == () and pool.free == 2 and tick == 3
    assert classes[2] == {0, 7040}                                            # a tick with two launch classes; slot 1 served sessions 1 and 2
    for k, T in enumerate(POOL_TOKENS):
        it = items[k]
        solo = net.stream_receiver(K, BOOKS, batch=1, **kw)
        want = []
        for c in range(T // 16):
            tp, ap = _chunk(it, c, False, 0)
            want.append(tuple(o.clone() for o in solo.push([tp], audio_packets=[ap])))
        if T % 16:
            tp, ap = _chunk(it, T // 16, True, 0)
            want.append(solo.finish([tp], [ap], tokens=T % 16))
        else:
            want.append(solo.finish())
        assert len(outs[k]) == len(want)
        for j, (g, w) in enumerate(zip(outs[k], want)):                       # tick by tick, both outputs
            assert g[0].shape == w[0].shape and torch.equal(g[0], w[0]), (k, j)
            assert g[1].shape == w[1].shape and torch.equal(g[1].view(torch.int32), w[1].view(torch.int32)), (k, j)
        ya = torch.cat([o[1] for o in outs[k]], dim=-1)
        assert torch.equal(ya.view(torch.int32), _want_audio(dev, T, 44100, 1).view(torch.int32)), k
        assert torch.equal(torch.cat([o[0] for o in outs[k]], dim=-1), it["whole"][0]), k
