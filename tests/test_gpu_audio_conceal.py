"""-m gpu: the receiver's audio concealment (key-masked attention, hold fill) against the existing unmasked kernels on compacted
K / V and against the numpy restatement of tests/audio_conceal_oracle.py.  Every comparison is an equality.

  1. mvq_attention_masked_f32: four shapes and the folded addressing of _rx_two_pass, six masks, NaN / 1e30 in the masked columns;
  2. mvq_attention_seq_masked_f32: three shapes (Tk = 130 spans three key tiles), NULL mask, refusals before any launch;
  3. mvq_hold_fill_f32: in place, with and without carry, -0 and NaN payloads;
  4. decode_latents(audio_conceal=) against the restatement; conceal="plc" under "mask" composed by hand;
  5. decompress_packets_av(audio_conceal=), also behind audio_fec=;
  6. StreamReceiver(audio=, audio_conceal=) against decompress_packets_av, eager and as a replayed graph."""
import numpy as np
import pytest
import torch

import audio_conceal_oracle as ac
import av_oracle as av
import golden_inputs as gi
import lossy_oracle as lo
import test_gpu_av as tav
import test_gpu_fec as tfec
from multimodal_vqvae_compression_audio_tactile_amd import packets

pytestmark = pytest.mark.gpu

f32 = np.float32
_REF = {}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _t(dev, *xs):
    return [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in xs]


def _masks(B, Tk, seed):
    """The six masks, uint8 [B, Tk]; present keys carry different nonzero values (any nonzero byte is "present")."""
    r = np.random.default_rng(seed)
    m = {"all": np.full((B, Tk), 1, np.uint8), "none": np.zeros((B, Tk), np.uint8)}
    m["first"] = np.zeros((B, Tk), np.uint8); m["first"][:, 0] = 32
    m["last"] = np.zeros((B, Tk), np.uint8); m["last"][:, Tk - 1] = 255
    m["alternating"] = np.tile((np.arange(Tk) % 2 == 0).astype(np.uint8) * 9, (B, 1))
    per = (r.uniform(size=(B, Tk)) < 0.5).astype(np.uint8) * r.integers(1, 256, size=(B, Tk)).astype(np.uint8)
    per[0, 0], per[1 % B, 0] = 0, (1 if B > 1 else 0)                    # rows differ: a wrong m_stride_b shows
    if B > 2:
        per[2] = 0                                                       # one item without a key among items with some
    m["per_item"] = per
    return m


def _qkv(B, C, Tq, Tk, seed, dev):
    r = np.random.default_rng(seed)
    return _t(dev, *(r.standard_normal((B, C, n)).astype(f32) for n in (Tq, Tk, Tk)))


def _compacted(attn, q, k, v, mask, heads):
    """The existing unmasked op per item on index_select-compacted K / V."""
    out = []
    for b in range(q.shape[0]):
        J = torch.nonzero(mask[b] != 0).reshape(-1)
        out.append(attn(q[b:b + 1].contiguous(), k[b:b + 1].index_select(2, J).contiguous(), v[b:b + 1].index_select(2, J).contiguous(), heads))
    return torch.cat(out, dim=0)


def _masked_chunk(q, k, v, mask, heads):
    from multimodal_vqvae_compression_audio_tactile_amd import ops
    B, C, Tq = q.shape
    Tk = k.shape[2]
    ctx = torch.full_like(q, float("nan"))                               # every element is written: garbage first
    return ops.attention_into_(ctx, q, k, v, heads, B, Tq, Tk, (C * Tq, Tq), (C * Tk, Tk), kmask=mask.reshape(-1), m_stride=Tk)


# ------------------------------------------------------------------------------------------------------- 1. the chunk kernel
CHUNK_SHAPES = [(3, 8, 128, 16, 16), (3, 8, 128, 1, 16), (2, 2, 8, 5, 64), (2, 2, 8, 3, 33)]


@pytest.mark.parametrize("B,H,dh,Tq,Tk", CHUNK_SHAPES)
def test_masked_chunk_attention_is_the_plain_kernel_on_compacted_keys(B, H, dh, Tq, Tk, dev, orc):
    from multimodal_vqvae_compression_audio_tactile_amd import ops
    q, k, v = _qkv(B, H * dh, Tq, Tk, B + H + dh + Tq + Tk, dev)
    plain = ops.attention(q, k, v, H)
    for name, mask in _masks(B, Tk, Tq + Tk).items():
        md, = _t(dev, mask)
        got = _masked_chunk(q, k, v, md, H)
        want = _compacted(ops.attention, q, k, v, md, H)
        assert torch.equal(got, want), name
        if name == "all":
            assert torch.equal(got, plain)
        if name == "none":
            assert not bool(got.any()) and not bool(torch.signbit(got).any())             # ctx = +0
        if name == "per_item" and B > 2:
            assert not bool(got[2].any()) and bool(got[0].any())
        if dh == 8 or Tq == 1:                                                            # two shapes also against the CPU oracle
            assert np.array_equal(got.cpu().numpy(), ac.masked_attention(orc, q.cpu().numpy(), k.cpu().numpy(), v.cpu().numpy(), mask, H)), name
        if name in ("alternating", "per_item"):                                           # a masked column never reaches the result
            for junk in (float("nan"), 1e30):
                absent = (md == 0)[:, None, :].expand_as(k)
                k2, v2 = torch.where(absent, torch.full_like(k, junk), k), torch.where(absent, torch.full_like(v, junk), v)
                assert torch.equal(_masked_chunk(q, k2, v2, md, H), want), (name, junk)
    # the C entry point with a NULL mask is the existing launch
    from multimodal_vqvae_compression_audio_tactile_amd import _lib
    raw = torch.full_like(q, float("nan"))
    rc = _lib.lib().mvq_attention_masked_f32(q.data_ptr(), k.data_ptr(), v.data_ptr(), None, raw.data_ptr(), B, H, dh, Tq, Tk, 0, 0, 0, 0, 0,
                                             _stream())
    assert rc == 0 and torch.equal(raw, plain)


def test_masked_chunk_attention_in_the_receivers_folded_layout(dev):
    """Groups of 16 inside [1, C, N], one mask buffer of group stride 16 for the chunk-as-batch call and the odd-chunk calls of both
    passes, q_col / k_col offsets."""
    from multimodal_vqvae_compression_audio_tactile_amd import ops
    B, NC, C, H, CH = 2, 3, 64, 2, 16
    G, P = B * NC, NC * CH
    N = B * P
    r = np.random.default_rng(5)
    Q, K, V = _t(dev, *(r.standard_normal((1, C, N)).astype(f32) for _ in range(3)))
    Q2, = _t(dev, r.standard_normal((1, C, G)).astype(f32))
    km = (r.uniform(size=N) < 0.6).astype(np.uint8) * 3
    km[CH:2 * CH] = 0                                                                     # group 1 has no key
    km_d, = _t(dev, km)

    def group(g, tq, tk, q_src, qcol):
        qg = q_src[:, :, qcol:qcol + tq].contiguous()
        cols = g * CH + torch.nonzero(km_d[g * CH:g * CH + tk] != 0).reshape(-1)
        return ops.attention(qg, K.index_select(2, cols).contiguous(), V.index_select(2, cols).contiguous(), H)

    # pass 1: every group, 16 queries and 16 keys
    ctx = torch.full_like(Q, float("nan"))
    ops.attention_into_(ctx, Q, K, V, H, G, CH, CH, (CH, N), (CH, N), kmask=km_d, m_stride=CH)
    for g in range(G):
        assert torch.equal(ctx[:, :, g * CH:(g + 1) * CH], group(g, CH, CH, Q, g * CH)), g
    assert not bool(ctx[:, :, CH:2 * CH].any())
    # the odd chunk c = 2 of every item: 5 queries, 14 keys, batch stride = one item's columns
    c, nt, ka = 2, 5, 14
    before = ctx.clone()
    ops.attention_into_(ctx, Q, K, V, H, B, nt, ka, (P, N), (P, N), q_col=c * CH, k_col=c * CH, kmask=km_d)
    for b in range(B):
        g = b * NC + c
        assert torch.equal(ctx[:, :, g * CH:g * CH + nt], group(g, nt, ka, Q, g * CH)), b
        assert torch.equal(ctx[:, :, g * CH + nt:(g + 1) * CH], before[:, :, g * CH + nt:(g + 1) * CH])      # nothing beyond is written
    # pass 2: one query per group
    ctx2 = torch.full_like(Q2, float("nan"))
    ops.attention_into_(ctx2, Q2, K, V, H, G, 1, CH, (1, G), (CH, N), kmask=km_d, m_stride=CH)
    for g in range(G):
        assert torch.equal(ctx2[:, :, g:g + 1], group(g, 1, CH, Q2, g)), g
    ops.attention_into_(ctx2, Q2, K, V, H, B, 1, ka, (NC, G), (P, N), q_col=c, k_col=c * CH, kmask=km_d)
    for b in range(B):
        g = b * NC + c
        assert torch.equal(ctx2[:, :, g:g + 1], group(g, 1, ka, Q2, g)), b
    from multimodal_vqvae_compression_audio_tactile_amd import MvqError
    with pytest.raises(MvqError, match="mask row"):
        ops.attention_into_(ctx, Q, K, V, H, G, CH, CH, (CH, N), (CH, N), kmask=km_d[:N - 1].contiguous())
    with pytest.raises(MvqError, match="kmask"):
        ops.attention_into_(ctx, Q, K, V, H, G, CH, CH, (CH, N), (CH, N), kmask=km_d.bool())


# ---------------------------------------------------------------------------------------------------- 2. the sequence kernel
def _seq_masks(B, Tk, seed):
    m = _masks(B, Tk, seed)
    if Tk > 128:                                                         # keys 64..127 entirely, and a partial first tile
        r = np.random.default_rng(seed)
        t = np.ones((B, Tk), np.uint8)
        t[:, 64:128] = 0
        t[:, :64] = r.uniform(size=(B, 64)) < 0.5
        t[:, 40] = 1
        m["tiles"] = t
        o = np.zeros((B, Tk), np.uint8)                                   # only the short last tile has keys
        o[:, 128:] = 1
        m["tail_tile"] = o
    return m


@pytest.mark.parametrize("B,H,dh,Tq,Tk", [(2, 8, 128, 75, 75), (1, 2, 8, 7, 130), (1, 2, 8, 4, 33)])
def test_masked_seq_attention_is_the_plain_kernel_on_compacted_keys(B, H, dh, Tq, Tk, dev):
    from multimodal_vqvae_compression_audio_tactile_amd import _lib, ops, torch_ops  # noqa: F401  (registers the operators)
    q, k, v = _qkv(B, H * dh, Tq, Tk, B + H + dh + Tq + Tk, dev)
    plain = ops.attention_seq(q, k, v, H)
    for name, mask in _seq_masks(B, Tk, Tq + Tk).items():
        md, = _t(dev, mask)
        got = ops.attention_seq(q, k, v, H, kmask=md)
        want = _compacted(ops.attention_seq, q, k, v, md, H)
        assert torch.equal(got, want), name
        if name == "all":
            assert torch.equal(got, plain)
        if name == "none":
            assert not bool(got.any()) and not bool(torch.signbit(got).any())
        if ops.attention_fits(dh, Tq, Tk):                                                # where the chunk kernel accepts the shape
            assert torch.equal(got, _masked_chunk(q, k, v, md, H)), name
        if name in ("per_item", "tiles"):
            for junk in (float("nan"), 1e30):
                absent = (md == 0)[:, None, :].expand_as(k)
                k2, v2 = torch.where(absent, torch.full_like(k, junk), k), torch.where(absent, torch.full_like(v, junk), v)
                assert torch.equal(ops.attention_seq(q, k2, v2, H, kmask=md), want), (name, junk)
        assert torch.equal(torch.ops.mi355x_vqvae.attention_seq_masked_f32(q, k, v, md, H), got)
    lib = _lib.lib()
    raw = torch.full_like(q, float("nan"))
    args = (B, H, dh, Tq, Tk, 0, 0, 0, 0)
    assert lib.mvq_attention_seq_masked_f32(q.data_ptr(), k.data_ptr(), v.data_ptr(), None, raw.data_ptr(), *args, 0, _stream()) == 0
    assert torch.equal(raw, plain)                                                        # a NULL mask is the existing launch
    # refused shapes: MVQ_EINVAL and no launch (the output keeps its garbage)
    raw.fill_(float("nan"))
    md, = _t(dev, np.ones((B, Tk), np.uint8))
    for bad in ((B, H, dh, Tq, 8193), (B, H, dh, 8193, Tk), (B, 0, dh, Tq, Tk), (B, 1, 100000, Tq, Tk), (-1, H, dh, Tq, Tk)):
        assert lib.mvq_attention_seq_masked_f32(q.data_ptr(), k.data_ptr(), v.data_ptr(), md.data_ptr(), raw.data_ptr(), *bad, 0, 0, 0, 0, Tk,
                                                _stream()) == -1, bad
    for bad in ((B, H, dh, Tq, 65), (B, H, dh, 65, min(Tk, 64)), (B, 1, 256, 64, 64)):
        assert lib.mvq_attention_masked_f32(q.data_ptr(), k.data_ptr(), v.data_ptr(), md.data_ptr(), raw.data_ptr(), *bad, 0, 0, 0, 0, Tk,
                                            _stream()) == -1, bad
    torch.cuda.synchronize()
    assert bool(torch.isnan(raw).all())
    from multimodal_vqvae_compression_audio_tactile_amd import MvqError
    with pytest.raises(MvqError, match="kmask"):
        ops.attention_seq(q, k, v, H, kmask=md[:, :Tk - 1].contiguous())


# --------------------------------------------------------------------------------------------------------- 3. the hold kernel
def _bits(x):
    return np.ascontiguousarray(x, f32).view(np.uint32)


@pytest.mark.parametrize("B,C,T", [(3, 1024, 37), (1, 64, 1), (2, 96, 130)])
def test_hold_fill_kernel_equals_numpy(B, C, T, dev):
    from multimodal_vqvae_compression_audio_tactile_amd import _lib, ops
    r = np.random.default_rng(B + C + T)
    x = r.standard_normal((B, C, T)).astype(f32)
    x.reshape(-1)[::7] = -0.0
    xb = _bits(x)
    xb.reshape(-1)[5::13] = 0x7FC12345                                                    # NaNs with a payload
    xb.reshape(-1)[6::17] = 0xFF800000                                                    # -inf
    x = xb.view(f32)
    carry = r.standard_normal((B, C)).astype(f32)
    carry[0, 0] = -0.0
    pats = {"none": np.zeros((B, T), np.uint8), "all": np.full((B, T), 32, np.uint8)}
    late = np.zeros((B, T), np.uint8); late[:, T // 2:] = r.integers(0, 2, size=(B, T - T // 2)) * 5; late[:, T - 1] = 0 if T > 2 else 1
    late[:, T // 2] = 255
    pats["late"] = late
    pats["runs"] = np.tile(((np.arange(T) // 3) % 2).astype(np.uint8), (B, 1))
    per = (r.uniform(size=(B, T)) < 0.4).astype(np.uint8); per[0] = 0
    pats["per_item"] = per
    if T > 64:
        far = np.zeros((B, T), np.uint8); far[:, 3] = 1; far[:, 64] = 1                   # a source two tiles back; one at a tile's first lane
        pats["far"] = far
    for name, valid in pats.items():
        for cr in (None, carry):
            want, want_carry = ac.hold_fill(x, valid, cr)
            xd, vd = _t(dev, x, valid)
            cd = None if cr is None else _t(dev, cr)[0]
            out = ops.hold_fill_(xd, vd, cd)
            assert out is xd                                                               # in place
            assert np.array_equal(_bits(xd.cpu().numpy()), _bits(want)), (name, cr is None)
            if cd is not None:                                                             # the one buffer is carry in and carry out
                assert np.array_equal(_bits(cd.cpu().numpy()), _bits(want_carry)), name
    # the C entry point; nothing beyond the tensor is written
    valid = pats["runs"]
    guard = torch.full((B * C * T + 64,), float("nan"), device=dev)
    guard[:B * C * T] = torch.from_numpy(x).to(dev).reshape(-1)
    vd, = _t(dev, valid)
    assert _lib.lib().mvq_hold_fill_f32(guard.data_ptr(), vd.data_ptr(), None, B, C, T, _stream()) == 0
    assert np.array_equal(_bits(guard[:B * C * T].cpu().numpy().reshape(B, C, T)), _bits(ac.hold_fill(x, valid)[0]))
    assert bool(torch.isnan(guard[B * C * T:]).all())
    from multimodal_vqvae_compression_audio_tactile_amd import MvqError
    xd, = _t(dev, x)
    for bad in (vd[:, :T - 1].contiguous() if T > 1 else vd.reshape(-1), vd.bool(), vd.cpu()):
        with pytest.raises(MvqError, match="valid"):
            ops.hold_fill_(xd, bad)
    with pytest.raises(MvqError, match="carry"):
        ops.hold_fill_(xd, vd, torch.zeros(B, C + 1, device=dev))
    with pytest.raises(MvqError, match="in place"):
        ops.hold_fill_(xd.double(), vd)


# -------------------------------------------------------------------------------------------------- 4. through decode_latents
def _model(dev, orc):
    if "model" not in _REF:
        sd = {k: v.numpy() for k, v in gi.model_state(7, 8, 512).items()}
        _REF["model"] = (tav._net(dev), sd, av.quantiser_of(orc, sd))
    return _REF["model"]


E2E = {"37": (3, 37, 37, None), "37_30": (3, 37, 30, None), "16": (1, 16, 16, [2])}     # B, Tlat, Ta, the items' loss kinds


def _e2e(name, dev, orc):
    """The transmitted arrays of a case, its loss on both streams and the restatement's z_run per mode, computed once."""
    if ("e2e", name) not in _REF:
        B, Tlat, Ta, kinds = E2E[name]
        net, sd, q3 = _model(dev, orc)
        a, t = tav._signals(dev, B, 320 * Tlat)
        _, codes, idx = net.encode_latents_with_indices(a, t)
        codes = codes[:, :, :Ta].contiguous()
        nav = ac.audio_loss(B, Ta, kinds=kinds)
        ac.check_audio_loss(nav, kinds=kinds)
        nbv = lo.loss_pattern("alternating", B, Tlat, 8)
        ch, ih = codes.cpu().numpy(), idx.cpu().numpy()
        want = {m: ac.receiver_av_conceal(orc, sd, q3, ch, ih, nbv, nav, m) for m in ("mask", "hold")}
        _REF[("e2e", name)] = (net, codes, idx, *_t(dev, nbv, nav), nbv, nav, want)
    return _REF[("e2e", name)]


@pytest.mark.parametrize("conceal", ["predict", "zero"])
@pytest.mark.parametrize("mode", ["mask", "hold"])
@pytest.mark.parametrize("name", list(E2E))
def test_decode_latents_audio_conceal_bit_exact(name, mode, conceal, dev, orc):
    net, codes, idx, nbv_d, nav_d, nbv, nav, want = _e2e(name, dev, orc)
    B, Tlat, Ta, kinds = E2E[name]
    got = net.decode_latents(codes, idx, nb_valid=nbv_d, na_valid=nav_d, conceal=conceal, audio_conceal=mode)
    ref = want[mode] if conceal == "predict" else want[mode] * (nbv != 0)[:, None, :].astype(f32)
    assert np.array_equal(got.cpu().numpy(), ref)
    zero = net.decode_latents(codes, idx, nb_valid=nbv_d, na_valid=nav_d, conceal=conceal)
    assert torch.equal(net.decode_latents(codes, idx, nb_valid=nbv_d, na_valid=nav_d, conceal=conceal, audio_conceal="zero"), zero)
    lossy_item = 1 if B > 1 else 0
    assert not torch.equal(got[lossy_item], zero[lossy_item])                             # a mode that ignores its mask fails here
    if B > 1:
        assert torch.equal(got[0], zero[0])                                               # item 0 lost nothing
    other = net.decode_latents(codes, idx, nb_valid=nbv_d, na_valid=nav_d, conceal=conceal, audio_conceal="hold" if mode == "mask" else "mask")
    assert not torch.equal(got[lossy_item], other[lossy_item])
    # nothing lost: every mode is na_valid=None
    full = torch.full_like(nav_d, 32)
    none = net.decode_latents(codes, idx, nb_valid=nbv_d, conceal=conceal)
    assert torch.equal(net.decode_latents(codes, idx, nb_valid=nbv_d, na_valid=full, conceal=conceal, audio_conceal=mode), none)
    assert torch.equal(net.decode_latents(codes, idx, nb_valid=nbv_d, conceal=conceal, audio_conceal=mode), none)
    # a thinned token is a valid lower-rate token in every mode: never concealed
    thin = torch.where(nav_d == 0, torch.full_like(nav_d, 1), nav_d)
    assert torch.equal(net.decode_latents(codes, idx, nb_valid=nbv_d, na_valid=thin, conceal=conceal, audio_conceal=mode),
                       net.decode_latents(codes, idx, nb_valid=nbv_d, na_valid=thin, conceal=conceal))
    # garbage in the codes that did not arrive changes nothing
    planted = torch.where((nav_d == 0)[:, None, :].expand_as(codes), torch.full_like(codes, 2 ** 40), codes)
    assert torch.equal(net.decode_latents(planted, idx, nb_valid=nbv_d, na_valid=nav_d, conceal=conceal, audio_conceal=mode), got)


def test_decode_latents_hold_piece_by_piece_with_the_carry(dev, orc):
    """qa_prev / qa_last_out mirror z_prev / z_last_out: pieces of whole chunks give the whole item's bits."""
    net, codes, idx, nbv_d, nav_d, nbv, nav, want = _e2e("37", dev, orc)
    B, C = 3, 1024
    z_c, qa_c = torch.zeros(B, C, device=dev), torch.zeros(B, C, device=dev)
    parts = []
    for s in (0, 16, 32):
        e = min(37, s + 16)
        parts.append(net.decode_latents(codes[:, :, s:e].contiguous(), idx[:, :, s:e].contiguous(), nb_valid=nbv_d[:, s:e].contiguous(),
                                        na_valid=nav_d[:, s:e].contiguous(), z_prev=z_c, z_last_out=z_c, audio_conceal="hold",
                                        qa_prev=qa_c, qa_last_out=qa_c))
    assert np.array_equal(torch.cat(parts, dim=2).cpu().numpy(), want["hold"])
    # separate in / out buffers: qa_prev stays as handed in
    prev, out = torch.randn(B, C, device=dev), torch.full((B, C), float("nan"), device=dev)
    keep = prev.clone()
    lost_first = nav_d[:, :16].clone(); lost_first[:, :4] = 0
    a = net.decode_latents(codes[:, :, :16].contiguous(), idx[:, :, :16].contiguous(), na_valid=lost_first, audio_conceal="hold", qa_prev=prev,
                           qa_last_out=out)
    assert torch.equal(prev, keep) and not bool(torch.isnan(out).any())
    b = net.decode_latents(codes[:, :, :16].contiguous(), idx[:, :, :16].contiguous(), na_valid=lost_first, audio_conceal="hold", qa_prev=prev)
    assert torch.equal(a, b) and torch.equal(prev, keep)
    assert not torch.equal(a, net.decode_latents(codes[:, :, :16].contiguous(), idx[:, :, :16].contiguous(), na_valid=lost_first, audio_conceal="hold"))


def test_decode_latents_plc_under_a_key_mask_is_the_predictor_composed_by_hand(dev, orc):
    from multimodal_vqvae_compression_audio_tactile_amd import ops
    net, codes, idx, nbv_d, nav_d, nbv, nav, want = _e2e("37", dev, orc)
    from test_gpu_lossy import _plc_for
    plc = _plc_for(net, dev)
    kw = dict(nb_valid=nbv_d, na_valid=nav_d, audio_conceal="mask")
    got = net.decode_latents(codes, idx, conceal="plc", plc=plc, **kw)
    z_run = net.decode_latents(codes, idx, **kw)
    lost = nbv_d == 0
    zt_in = ops.plc_mask_fill(z_run, None, lost)[0]
    qa = net.A_QUANT.from_codes(codes, nq_valid=nav_d)[0]
    pr, L = plc.predict, plc.predict._lin
    w = lambda m: (m.weight.detach(), m.bias.detach())
    q = ops.layernorm_c(zt_in, *w(pr.ln_q), pe=pr.pos.pe, eps=pr.ln_q.eps)
    kv = ops.layernorm_c(qa, *w(pr.ln_kv), pe=pr.pos.pe, eps=pr.ln_kv.eps)
    Q, K, V = L["q"](q), L["k"](kv), L["v"](kv)
    ctx = _compacted(ops.attention_seq, Q, K, V, nav_d, pr.h)                             # the unmasked kernel on the arrived keys
    assert torch.equal(ctx, ops.attention_seq(Q, K, V, pr.h, kmask=nav_d))
    y1 = L["o"](ctx, residual=q)
    hdn = L["f1"](ops.layernorm_c(y1, *w(pr.ffn[0]), eps=pr.ffn[0].eps), gelu=True)
    z_pred = L["f3"](hdn, residual=y1)
    with torch.no_grad():
        assert torch.equal(plc.predict(zt_in, qa, key_mask=nav_d), z_pred)
    from multimodal_vqvae_compression_audio_tactile_amd import MvqError
    with pytest.raises(MvqError, match="inference only"):                                 # autograd is recording here
        plc.predict(zt_in, qa, key_mask=nav_d)
    assert torch.equal(got, ops.plc_mask_fill(z_run, z_pred, lost, want_zt_in=False)[1])
    assert not torch.equal(got, net.decode_latents(codes, idx, conceal="plc", plc=plc, nb_valid=nbv_d, na_valid=nav_d))
    # under "hold" the PLC predictor is handed the held qa
    held = ops.hold_fill_(qa.clone(), nav_d)
    zh = net.decode_latents(codes, idx, nb_valid=nbv_d, na_valid=nav_d, audio_conceal="hold")
    with torch.no_grad():
        zp_h = plc.predict(ops.plc_mask_fill(zh, None, lost)[0], held)
    assert torch.equal(net.decode_latents(codes, idx, conceal="plc", plc=plc, nb_valid=nbv_d, na_valid=nav_d, audio_conceal="hold"),
                       ops.plc_mask_fill(zh, zp_h, lost, want_zt_in=False)[1])


# --------------------------------------------------------------------------------------------------- 5. the whole-item link
def _gathered(rx, arx, info, ainfo, dev):
    hi, hv, hc, ha = [], [], [], []
    for b in range(len(rx)):
        i_b, v_b = packets.unpack_bodies(*packets.gather(rx[b], info), info)
        c_b, a_b = packets.unpack_bodies(*packets.gather(arx[b], ainfo), ainfo)
        hi.append(i_b); hv.append(v_b); hc.append(c_b); ha.append(a_b)
    return _t(dev, np.stack(hi, axis=1), np.stack(hv).astype(np.uint8), np.stack(hc, axis=0), np.stack(ha).astype(np.uint8))


@pytest.mark.parametrize("mode", ["mask", "hold"])
def test_decompress_packets_av_audio_conceal(mode, dev):
    net = tav._net(dev)
    B, Tlat = 3, 37
    a, t = tav._signals(dev, B, 320 * Tlat)
    rate, arate = tav.RATES["tol2"]
    infos, pk, ainfos, apk = net.compress_packets_av(a, t, rate=rate, audio_rate=arate)
    info, ainfo = infos[0], ainfos[0]
    rx = [tav._channel(pk[b], info, 10 * b + 1)[0] for b in range(B)]                     # dropped, thinned, reversed, duplicated
    arx = [tav._channel(apk[b], ainfo, 10 * b + 2)[0] for b in range(B)]
    idx_r, nbv, codes_r, nav = _gathered(rx, arx, info, ainfo, dev)
    assert int((nav == 0).sum()) > 0 and int((nbv == 0).sum()) > 0 and len(set(nav.reshape(-1).tolist())) >= 3
    for conceal in ("predict", "zero"):
        y, lost, alost = net.decompress_packets_av(infos, rx, ainfos, arx, conceal=conceal, audio_conceal=mode)
        assert torch.equal(y, net.decode(codes_r, idx_r, nb_valid=nbv, na_valid=nav, conceal=conceal, audio_conceal=mode)), conceal
        assert torch.equal(lost, nbv == 0) and torch.equal(alost, nav == 0)
        assert not torch.equal(y, net.decompress_packets_av(infos, rx, ainfos, arx, conceal=conceal)[0])
    zero = net.decompress_packets_av(infos, rx, ainfos, arx)
    same = net.decompress_packets_av(infos, rx, ainfos, arx, audio_conceal="zero")
    assert all(torch.equal(p, q) for p, q in zip(zero, same))
    # nothing lost: every mode is the lossless result
    assert torch.equal(net.decompress_packets_av(infos, pk, ainfos, apk, audio_conceal=mode)[0], net.decompress_packets_av(infos, pk, ainfos, apk)[0])


@pytest.mark.parametrize("mode", ["mask", "hold"])
def test_decompress_packets_av_audio_conceal_behind_fec(mode, dev):
    """What the parity recovers is not lost and is not concealed; what stays lost is."""
    net = tav._net(dev)
    B, Tlat = 3, 37
    a, t = tav._signals(dev, B, 320 * Tlat)
    infos, pk, ainfos, apk, par, apar = net.compress_packets_av(a, t, rate=tfec.RATE, audio_rate=tfec.ARATE, fec=tfec.FEC, audio_fec=tfec.AFEC)
    info, ainfo = infos[0], ainfos[0]
    rx, rxp, fixed, _ = tfec._lossy(pk, par, info, tfec.FEC, 1)
    n_lost = lambda lists: sum(int((packets.gather(lists[b], ainfo)[1] == 0).sum()) for b in range(B))
    for seed in range(2, 10):                                # the first seeded channel (numpy rule alone) on which some lost audio
        arx, arxp, afixed, _ = tfec._lossy(apk, apar, ainfo, tfec.AFEC, seed)             # packets come back and some stay lost
        if 0 < n_lost(afixed) < n_lost(arx):
            break
    else:
        raise AssertionError("no seed gives both a recovered and an unrecovered audio packet")
    y, lost, alost = net.decompress_packets_av(infos, rx, ainfos, arx, audio_fec=tfec.AFEC, audio_fec_packets=arxp, audio_conceal=mode)
    want = net.decompress_packets_av(infos, rx, ainfos, afixed, audio_conceal=mode)
    assert torch.equal(y, want[0]) and torch.equal(lost, want[1]) and torch.equal(alost, want[2])
    plain_lost = net.decompress_packets_av(infos, rx, ainfos, arx)[2]
    assert 0 < int(alost.sum()) < int(plain_lost.sum())
    idx_r, nbv, codes_r, nav = _gathered(rx, afixed, info, ainfo, dev)
    assert torch.equal(alost, nav == 0)
    assert torch.equal(y, net.decode(codes_r, idx_r, nb_valid=nbv, na_valid=nav, audio_conceal=mode))
    assert not torch.equal(y, net.decompress_packets_av(infos, rx, ainfos, arx, audio_fec=tfec.AFEC, audio_fec_packets=arxp)[0])


# ------------------------------------------------------------------------------------------------------------ 6. streaming
def _audio_drops(apk, T):
    """Item 0 loses its first packet, ALL of chunk 1 (so a hold crosses two chunk borders) and a different packet of every later
    chunk; item 1 loses every other packet and the last one."""
    P = len(apk[0])
    drop0 = {0} | set(range(8, 16)) | {8 * c + (c % 8) for c in range(2, (T + 15) // 16)}
    drop1 = set(range(1, P, 2)) | {P - 1}
    keep = lambda lst, drop: [p for s, p in enumerate(lst) if s not in drop][::-1]           # and reordered
    return [keep(apk[0], drop0), keep(apk[1], drop1)]


@pytest.mark.parametrize("Tlat,graph", [(75, False), (75, True), (37, False)])
@pytest.mark.parametrize("mode", ["mask", "hold"])
def test_stream_receiver_audio_conceal_equals_the_whole_item_call(mode, Tlat, graph, dev):
    net = tav._net(dev)
    B = 2
    a, t = tav._signals(dev, B, 320 * Tlat)
    key = ("stream", Tlat)
    if key not in _REF:
        infos, pk, ainfos, apk = net.compress_packets_av(a, t)
        rx_pk = [tav._channel(pk[b], infos[0], 10 * b + 1)[0] for b in range(B)]
        _REF[key] = (infos[0], ainfos[0], rx_pk, _audio_drops(apk, Tlat))
    info, ainfo, rx_pk, rx_apk = _REF[key]
    seq = lambda p: int.from_bytes(bytes(p)[3:7], "little")
    counts = packets.gather(rx_apk[0], ainfo)[1]
    assert not counts[8:16].any() and counts[16:24].any()                                 # a whole chunk of audio is gone
    if Tlat == 75:                                                                        # the replays see different loss patterns
        assert not np.array_equal(counts[16:24] != 0, counts[24:32] != 0)
    want, lost, alost = net.decompress_packets_av([info] * B, rx_pk, [ainfo] * B, rx_apk, audio_conceal=mode)
    assert bool(alost[0, 16:32].all()) and not torch.equal(want, net.decompress_packets_av([info] * B, rx_pk, [ainfo] * B, rx_apk)[0])
    rx = net.stream_receiver(512, 8, batch=B, graph=graph, audio=(1024, 32), audio_conceal=mode)
    assert (rx.qa_carry is not None) == (mode == "hold")
    ys = []
    for c in range(info.T // 16):
        pick = lambda lists: [[p for p in lists[b] if 8 * c <= seq(p) < 8 * c + 8] for b in range(B)]
        ys.append(rx.push(pick(rx_pk), audio_packets=pick(rx_apk)).clone())
    tail = lambda lists: [[p for p in lists[b] if seq(p) >= 8 * (info.T // 16)] for b in range(B)]
    ys.append(rx.finish(tail(rx_pk), tail(rx_apk), tokens=info.T % 16))
    got = torch.cat(ys, dim=-1)
    assert got.shape == want.shape and torch.equal(got, want)
    if graph:
        assert rx._g is not None and isinstance(rx._g[0], torch.cuda.CUDAGraph)
