"""-m gpu: fine-tuning the tactile decoder -- the weight-gradient kernels (csrc/conv_wgrad.hip), Decoder.backward_params and the
autograd path, against torch autograd in float64 on oracle/dac24_torch.py (kernel cases: F.conv1d / F.conv_transpose1d in float64),
computed on the CPU.

Tolerance: the suite's bar and helpers (tests/test_gpu_train_shapes.py).  Relative L2 <= TOL = 2e-4 per tensor, and a LOCAL bound:
the worst row of a weight gradient (dW, dv) and the worst element against the tensor's RMS (db, dalpha, dg) <= WORST_K / WORST_D.  Beside
every HIP figure the same error of the restatement run in fp32 on the CPU is printed (`fp32`).
Measured on the MI355X (largest over every case; `fp32` = the restatement in fp32 on the CPU):
  kernel cases    dW rel 3.3e-7 (fp32 1.4e-6), worst row 6.6e-7 (1.8e-6), worst column 4.4e-7 (2.5e-6); dalpha per element 1.2e-6 (1.0e-6);
                  db 2.5e-7 (2.7e-7); dg 7.7e-7 (2.6e-6); dv worst row 1.4e-7 (4.5e-7)        -> WORST_K = 1.2e-5 = 10 x 1.2e-6
  whole decoders  dv worst row 2.9e-5 (fp32 2.6e-5: model.0 of the full decoder, the gradient having crossed every layer in fp32);
                  dalpha per element 1.9e-5 (9.7e-6); dg per element 1.6e-5 (1.3e-5); db 1.4e-5 (1.1e-5); gz rel 1.6e-6 (1.1e-6);
                  dg rel on the small decoder 1.98e-4 (fp32 2.18e-4: s = <dW, v> cancels, in either fp32 arithmetic)
                                                                                              -> WORST_D = TOL (10 x 2.9e-5 is above it)"""
import gc
import math

import pytest
import torch
import torch.nn.functional as F

import decoder_finetune_cases as fc
from test_gpu_train_shapes import TOL, rel, worst_elem, worst_slice

pytestmark = pytest.mark.gpu
WORST_K = 1.2e-5         # local bound of the kernel cases
WORST_D = TOL            # ... of the whole-decoder cases
EINVAL = -1
NAN = float("nan")
O = fc.O
FIG = {}                 # kind -> [largest HIP figure, largest fp32-restatement figure], printed by every test that adds to it


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _lib():
    from multimodal_vqvae_compression_audio_tactile_amd import _lib
    return _lib.lib()


def _note(kind, hip, ref32):
    cur = FIG.setdefault(kind, [0.0, 0.0])
    cur[0], cur[1] = max(cur[0], hip), max(cur[1], ref32 if ref32 is not None else 0.0)


def _report(*kinds):
    for k in kinds or sorted(FIG):
        if k in FIG:
            print(f"  {k:26s} HIP {FIG[k][0]:.2e}   fp32 {FIG[k][1]:.2e}")


def check(name, got, want, want32=None, rows=False, elem=False, kind=None, worst=None):
    """rel L2 <= TOL; rows: worst dim-0 row <= WORST; elem: worst element / RMS <= WORST.  want32: the fp32 restatement's result."""
    got = got.detach().cpu()
    assert got.shape == want.shape, (name, got.shape, want.shape)
    assert torch.isfinite(got).all(), name
    kind = kind or name.split()[0]
    r = rel(got, want)
    _note(kind + " rel", r, rel(want32, want) if want32 is not None else None)
    w = None
    if rows:
        w = worst_slice(got, want, 0)
        _note(kind + " row", w, worst_slice(want32, want, 0) if want32 is not None else None)
    if elem:
        w = worst_elem(got, want)
        _note(kind + " elem", w, worst_elem(want32, want) if want32 is not None else None)
    assert r <= TOL, f"{name}: relative L2 error {r:.3g} > {TOL}"
    if w is not None:
        worst = WORST_K if worst is None else worst
        assert w <= worst, f"{name}: worst {'row' if rows else 'element'} error {w:.3g} > {worst}"


# ------------------------------------------------------------------------------------------------------------ conv weight gradient
def _snake_ref(x, alpha):
    return O.snake(x, alpha.reshape(1, -1, 1))


def _wgrad_want(gy, a, alpha, ks, stride, dil, pad, transposed, op, dtype):
    """dW by autograd of the forward conv (linear in w, so w = 0 will do) in `dtype` on the CPU."""
    gy, a = gy.to(dtype), a.to(dtype)
    if alpha is not None:
        a = _snake_ref(a, alpha.to(dtype))
    cout, cin = gy.shape[1], a.shape[1]
    w = torch.zeros((cin, cout, ks) if transposed else (cout, cin, ks), dtype=dtype, requires_grad=True)
    y = F.conv_transpose1d(a, w, stride=stride, padding=pad, output_padding=op) if transposed else F.conv1d(a, w, padding=pad, dilation=dil)
    assert y.shape == gy.shape, (y.shape, gy.shape)
    (y * gy).sum().backward()
    return w.grad


def _wgrad_raw(gy, a, alpha, ks, stride, dil, pad, transposed, tout=None, ws_short=0):
    """The C entry point on an output and a workspace filled with NaN -> (rc, dw, workspace bytes)."""
    lib = _lib()
    B, cout, to = gy.shape
    _, cin, tin = a.shape
    geo = (B, cin, tin, cout, to if tout is None else tout, ks, stride, dil, pad, int(transposed))
    n = lib.mvq_conv1d_wgrad_workspace_bytes(*geo)
    dw = torch.full((cin, cout, ks) if transposed else (cout, cin, ks), NAN, device=gy.device)
    ws = torch.full(((n + 3) // 4 + 1,), NAN, device=gy.device)
    rc = lib.mvq_conv1d_wgrad_f32(gy.data_ptr(), a.data_ptr(), None if alpha is None else alpha.data_ptr(), dw.data_ptr(), ws.data_ptr(),
                                  n - ws_short, *geo, _stream())
    return rc, dw, n


def _alpha(c, gen):
    al = torch.exp(0.5 * torch.randn(c, generator=gen))
    al[0], al[-1] = 1e-3, 8.0
    return al


def _wgrad_case(B, cin, cout, T, ks, stride, dil, pad, transposed, snake, dev, op=0, seed=0):
    from multimodal_vqvae_compression_audio_tactile_amd import ops
    gen = torch.Generator().manual_seed(seed * 7919 + B * 131 + T)
    tout = (T - 1) * stride - 2 * pad + ks + op if transposed else T + 2 * pad - dil * (ks - 1)
    a = torch.randn(B, cin, T, generator=gen)
    gy = torch.randn(B, cout, tout, generator=gen)
    alpha = _alpha(cin, gen) if snake else None
    want = _wgrad_want(gy, a, alpha, ks, stride, dil, pad, transposed, op, torch.float64)
    want32 = _wgrad_want(gy, a, alpha, ks, stride, dil, pad, transposed, op, torch.float32)
    gd, ad, ald = gy.to(dev), a.to(dev), None if alpha is None else alpha.to(dev)
    rc, dw, _ = _wgrad_raw(gd, ad, ald, ks, stride, dil, pad, transposed)
    assert rc == 0, _lib().mvq_last_error()
    rc2, dw2, _ = _wgrad_raw(gd, ad, ald, ks, stride, dil, pad, transposed)
    again = ops.conv1d_wgrad(gd, ad, ks, stride, dil, pad, transposed=transposed, snake_alpha=ald)
    tag = f"dW {'T' if transposed else 'C'} B={B} {cin}->{cout} T={T} k{ks} s{stride} d{dil} op{op} snake={snake}"
    assert rc2 == 0 and torch.equal(dw, dw2) and torch.equal(dw, again), f"{tag}: two runs differ"        # determinism; wrapper == raw
    check(tag, dw, want, want32, rows=True, kind="dW")
    # the other axis of the weight as well: one input (conv) / output (transposed) channel off shows in its column, not in a row
    w = worst_slice(dw.cpu(), want, 1)
    _note("dW col", w, worst_slice(want32, want, 1))
    assert w <= WORST_K, f"{tag}: worst dim-1 slice {w:.3g} > {WORST_K}"


K7_CH = [(32, 32), (96, 96), (64, 160)]


@pytest.mark.parametrize("dil", [1, 3, 9])
@pytest.mark.parametrize("cin,cout", K7_CH, ids=[f"{i}x{o}" for i, o in K7_CH])
def test_wgrad_conv_k7(cin, cout, dil, dev):
    """Conv1d k7, pad = 3 dil: T below the padding (taps past both ends), T no multiple of the 64-token chunk or of 4, B in {1, 3},
    with and without Snake staged on load."""
    for T in (1, 5, 16, 75, 203):
        for B in (1, 3):
            for snake in (False, True):
                _wgrad_case(B, cin, cout, T, 7, 1, dil, 3 * dil, False, snake, dev, seed=dil)
    _report("dW rel", "dW row", "dW col")


def test_wgrad_conv_k7_split_k_with_a_ragged_last_chunk(dev):
    """B = 2, C = 32, T = 6001: 188 chunks in 188 splits, the last chunk of each item one token long; and 2 x 96 x 24 000 / 4 at
    dil 9 with more chunks than splits (several chunks per split)."""
    assert _lib().mvq_conv1d_wgrad_workspace_bytes(2, 32, 6001, 32, 6001, 7, 1, 1, 3, 0) == 188 * 32 * 32 * 7 * 4
    _wgrad_case(2, 32, 32, 6001, 7, 1, 1, 3, False, True, dev)
    _wgrad_case(2, 32, 32, 6001, 7, 1, 9, 27, False, False, dev)
    assert _lib().mvq_conv1d_wgrad_workspace_bytes(3, 96, 6000, 96, 6000, 7, 1, 9, 27, 0) == 256 * 96 * 96 * 7 * 4      # 282 chunks, 256 splits
    _wgrad_case(3, 96, 96, 6000, 7, 1, 9, 27, False, True, dev)
    _report("dW rel", "dW row", "dW col")


@pytest.mark.parametrize("c", [96, 192])
def test_wgrad_conv_k1(c, dev):
    for T in (5, 75):
        for B in (1, 3):
            for snake in (False, True):
                _wgrad_case(B, c, c, T, 1, 1, 1, 0, False, snake, dev, seed=c)
    _report("dW rel", "dW row", "dW col")


def test_wgrad_final_conv_reduction_form(dev):
    """96 -> 1, k7 (dW[1][96][7]): the reduction form; T = 2500 crosses its 1024-token chunk and splits."""
    for T in (7, 203, 2500):
        for B in (1, 3):
            for snake in (False, True):
                _wgrad_case(B, 96, 1, T, 7, 1, 1, 3, False, snake, dev, seed=T)
    _report("dW rel", "dW row", "dW col")


def test_wgrad_head_conv(dev):
    """1024 -> 64, k7 (model.0's shape class: no Snake in front, many input channels, few tokens)."""
    for T in (1, 5):
        for B in (1, 3):
            _wgrad_case(B, 1024, 64, T, 7, 1, 1, 3, False, False, dev, seed=T)
    _report("dW rel", "dW row", "dW col")


@pytest.mark.parametrize("stride", [2, 4, 5, 8])
def test_wgrad_conv_transpose(stride, dev):
    """ConvTranspose1d ks = 2 stride, pad = ceil(stride / 2), output_padding in {0, stride % 2}."""
    for cin, cout in ((64, 32), (192, 96)):
        for T in (1, 5, 75):
            for B in (1, 3):
                for op in sorted({0, stride % 2}):
                    _wgrad_case(B, cin, cout, T, 2 * stride, stride, 1, math.ceil(stride / 2), True, (T + B) % 2 == 0, dev, op=op, seed=stride)
    _report("dW rel", "dW row", "dW col")


def test_wgrad_refusals_leave_the_output_untouched(dev):
    """A mismatched tout, a workspace one byte short and ks != 2 stride for the transposed form: MVQ_EINVAL, dW still all NaN."""
    g = torch.randn(2, 32, 6001, device=dev)
    for kw in (dict(tout=6000), dict(ws_short=1)):
        rc, dw, n = _wgrad_raw(g, g, None, 7, 1, 1, 3, False, **kw)
        assert rc == EINVAL and bool(torch.isnan(dw).all()) and n == (0 if "tout" in kw else 188 * 32 * 32 * 7 * 4), kw
    a, gy = torch.randn(2, 64, 75, device=dev), torch.randn(2, 32, 150, device=dev)
    rc, dw, _ = _wgrad_raw(gy, a, None, 5, 2, 1, 1, True)
    assert rc == EINVAL and bool(torch.isnan(dw).all())
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------- Snake backward
@pytest.mark.parametrize("B,C,T", [(1, 96, 5), (3, 96, 203), (3, 192, 75), (2, 32, 4500)])
def test_snake_bwd(B, C, T, dev):
    """gx is bit for bit the fused dgrad epilogue (with and without the skip gradient); dalpha against float64; alpha = 1e-4 and 30
    among the channels; T = 4500 spans three 2048-token slabs.  Called twice: the same bits."""
    from multimodal_vqvae_compression_audio_tactile_amd import ops
    gen = torch.Generator().manual_seed(B * 1000 + C + T)
    x = 1.5 * torch.randn(B, C, T, generator=gen)
    gy = torch.randn(B, C, T, generator=gen)
    res = torch.randn(B, C, T, generator=gen)
    alpha = torch.exp(0.5 * torch.randn(C, generator=gen))
    alpha[1], alpha[2] = 1e-4, 30.0
    w = torch.randn(C, C, 1, generator=gen) / math.sqrt(C)
    xd, gd, rd, ad = x.to(dev), gy.to(dev), res.to(dev), alpha.to(dev)
    wp = ops.pack_conv1d_dgrad(w.to(dev))
    gs = ops.conv1d_dgrad(gd, wp, C, T, 1)                                      # the gradient at the Snake's output, no epilogue
    lib = _lib()
    for r in (None, rd):
        fused = ops.conv1d_dgrad(gd, wp, C, T, 1, dsnake_src=xd, dsnake_alpha=ad, residual=r)
        n = lib.mvq_channel_reduce_workspace_bytes(B, C, T)
        outs = []
        for _ in range(2):
            gx, da, ws = torch.full_like(xd, NAN), torch.full((C,), NAN, device=dev), torch.full((n // 4 + 1,), NAN, device=dev)
            rc = lib.mvq_snake_bwd_f32(gs.data_ptr(), xd.data_ptr(), ad.data_ptr(), None if r is None else r.data_ptr(), gx.data_ptr(),
                                       da.data_ptr(), ws.data_ptr(), n, B, C, T, _stream())
            assert rc == 0, lib.mvq_last_error()
            outs.append((gx, da))
        assert torch.equal(outs[0][0], fused), f"gx differs from the fused epilogue (residual={r is not None})"
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
        gx2, da2 = ops.snake_bwd(gs, xd, ad, residual=r)
        assert torch.equal(gx2, fused) and torch.equal(da2, outs[0][1])
        gx3, none = ops.snake_bwd(gs, xd, ad, residual=r, need_dalpha=False)
        assert none is None and torch.equal(gx3, fused)
    want = {}
    for dt in (torch.float64, torch.float32):
        al = alpha.to(dt).requires_grad_(True)
        (_snake_ref(x.to(dt), al) * gs.cpu().to(dt)).sum().backward()
        want[dt] = al.grad
    check(f"dalpha B={B} C={C} T={T}", outs[0][1], want[torch.float64], want[torch.float32], elem=True)
    # a one-byte-short workspace: refused, outputs untouched
    gx, da = torch.full_like(xd, NAN), torch.full((C,), NAN, device=dev)
    ws = torch.full((n // 4 + 1,), NAN, device=dev)
    assert lib.mvq_snake_bwd_f32(gs.data_ptr(), xd.data_ptr(), ad.data_ptr(), None, gx.data_ptr(), da.data_ptr(), ws.data_ptr(), n - 1, B, C, T,
                                 _stream()) == EINVAL
    assert bool(torch.isnan(gx).all()) and bool(torch.isnan(da).all())
    _report("dalpha rel", "dalpha elem")


@pytest.mark.parametrize("B,C,T", [(1, 1, 7), (3, 96, 203), (2, 1536, 5), (2, 32, 4500)])
def test_bias_grad(B, C, T, dev):
    from multimodal_vqvae_compression_audio_tactile_amd import ops
    gy = torch.randn(B, C, T, generator=torch.Generator().manual_seed(C + T)) + 0.1
    gd = gy.to(dev)
    lib = _lib()
    n = lib.mvq_channel_reduce_workspace_bytes(B, C, T)
    db, ws = torch.full((C,), NAN, device=dev), torch.full((n // 4 + 1,), NAN, device=dev)
    assert lib.mvq_bias_grad_f32(gd.data_ptr(), db.data_ptr(), ws.data_ptr(), n, B, C, T, _stream()) == 0
    assert torch.equal(db, ops.bias_grad(gd))
    check(f"db B={B} C={C} T={T}", db, gy.double().sum(dim=(0, 2)), gy.sum(dim=(0, 2)), elem=True)
    _report("db rel", "db elem")


# -------------------------------------------------------------------------------------------------------------- weight-norm backward
@pytest.mark.parametrize("rows,cols", [(1, 672), (96, 672), (1536, 12288)])
def test_weight_norm_bwd(rows, cols, dev):
    """(dg, dv) of w = g v / ||v|| per dim-0 row against float64 autograd; one row has g = 0 (dv = 0 there, dg is not)."""
    from multimodal_vqvae_compression_audio_tactile_amd import ops
    gen = torch.Generator().manual_seed(rows + cols)
    ks = 7 if cols % 7 == 0 else 16
    v = torch.randn(rows, cols // ks, ks, generator=gen) / math.sqrt(cols)
    g = torch.exp(0.3 * torch.randn(rows, 1, 1, generator=gen))
    g[rows // 2] = 0.0
    dw = torch.randn(rows, cols // ks, ks, generator=gen)
    want = {}
    for dt in (torch.float64, torch.float32):
        vr, gr = v.to(dt).requires_grad_(True), g.to(dt).requires_grad_(True)
        w = gr * vr / vr.reshape(rows, -1).norm(dim=1).reshape(rows, 1, 1)
        (w * dw.to(dt)).sum().backward()
        want[dt] = (gr.grad, vr.grad)
    lib = _lib()
    vd, gd, dd = v.to(dev), g.to(dev), dw.to(dev)
    outs = []
    for _ in range(2):
        dg, dv = torch.full_like(gd, NAN), torch.full_like(vd, NAN)
        assert lib.mvq_weight_norm_bwd_f32(dd.data_ptr(), vd.data_ptr(), gd.data_ptr(), dg.data_ptr(), dv.data_ptr(), rows, cols, _stream()) == 0
        outs.append((dg, dv))
    dg, dv = outs[0]
    assert torch.equal(dg, outs[1][0]) and torch.equal(dv, outs[1][1])
    dg2, dv2 = ops.weight_norm_bwd(dd, vd, gd)
    assert torch.equal(dg2, dg) and torch.equal(dv2, dv)
    assert ops.weight_norm_bwd(dd, vd, gd, need_dv=False)[1] is None and torch.equal(ops.weight_norm_bwd(dd, vd, gd, need_dg=False)[1], dv)
    assert not bool(dv[rows // 2].any())
    check(f"dg {rows}x{cols}", dg, want[torch.float64][0], want[torch.float32][0], elem=True)
    keep = [r for r in range(rows) if r != rows // 2] or [0]                      # the g = 0 row is exactly 0 on both sides
    if rows > 1:
        check(f"dv {rows}x{cols}", dv[keep], want[torch.float64][1][keep], want[torch.float32][1][keep], rows=True)
    assert torch.equal(dv[rows // 2].cpu(), want[torch.float32][1][rows // 2] * 0)
    _report("dg rel", "dg elem", "dv rel", "dv row")


# ------------------------------------------------------------------------------------------------------------------- whole decoders
def _param_kind(name):
    return name.rsplit(".", 1)[-1]


def _check_param_grads(grads, ref64, ref32, names, tag):
    r64, r32 = dict(ref64.named_parameters()), dict(ref32.named_parameters())
    for n in names:
        got, want, want32 = grads[n], r64[n].grad, r32[n].grad.double()
        assert tuple(got.shape) == tuple(want.shape), (n, got.shape, want.shape)
        kind = _param_kind(n)
        if kind == "weight_v":
            check(f"{tag} {n}", got, want, want32, rows=want.shape[0] > 1, kind="dec dv", worst=WORST_D)
        else:
            check(f"{tag} {n}", got.reshape(-1), want.reshape(-1), want32.reshape(-1), elem=want.numel() > 1, kind="dec d" + kind, worst=WORST_D)


def _oracle_grads(sd, z, gy, kw):
    refs = []
    for dt in (torch.float64, torch.float32):
        ref = fc.oracle_decoder(sd, dt, **kw)
        zr = z.to(dt).requires_grad_(True)
        (ref(zr) * gy.to(dt)).sum().backward()
        refs.append((ref, zr.grad))
    return refs


@pytest.fixture(scope="module")
def small(dev):
    from multimodal_vqvae_compression_audio_tactile_amd import Decoder
    sd = fc.small_state()
    dec = Decoder(**fc.SMALL)
    dec.load_state_dict(sd, strict=True)
    return sd, dec.to(dev)


@pytest.mark.parametrize("B,T", [(1, 5), (3, 11)])
def test_small_decoder_every_gradient(small, B, T, dev):
    """Decoder.backward_params on the small decoder: every parameter gradient and gz against float64 autograd of the restatement
    loaded with the same state dict; every named parameter present with its shape; gz bit-equal to backward_input's."""
    sd, dec = small
    for p in dec.parameters():
        p.requires_grad_(True)
    gen = torch.Generator().manual_seed(B * 100 + T)
    z = 0.5 * torch.randn(B, fc.SMALL["input_channel"], T, generator=gen)
    gy = torch.randn(B, 1, fc.out_len(T, fc.SMALL["rates"]), generator=gen)
    (ref64, gz64), (ref32, gz32) = _oracle_grads(sd, z, gy, fc.SMALL)
    zd, gd = z.to(dev), gy.to(dev)
    y, saved = dec._forward_saving_plan(zd)
    assert rel(y, ref64(z.double())) < 1e-5
    saved["z"] = zd
    gz, grads = dec.backward_params(saved, gd)
    assert not [k for k in saved if k not in ("z_len",)], list(saved)           # every saved tensor was released
    names = [n for n, _ in dec.named_parameters()]
    assert sorted(grads) == sorted(names)
    for n, p in dec.named_parameters():
        assert grads[n].shape == p.shape, n
    _check_param_grads(grads, ref64, ref32, names, f"small B={B} T={T}")
    check("dec gz", gz, gz64, gz32.double(), kind="dec gz")
    _, saved2 = dec._forward_saving_plan(zd)
    assert torch.equal(gz, dec.backward_input(saved2, gd))
    # through autograd: the same tensors land in .grad, z needs no gradient for it
    for p in dec.parameters():
        p.grad = None
    with torch.enable_grad():
        dec(zd).backward(gd)
    for n, p in dec.named_parameters():
        assert p.grad is not None and torch.equal(p.grad, grads[n]), n
    _report()


def test_full_decoder_sampled_gradients(dev):
    """The full-size Decoder, synth.decoder_state(74), B = 1, T = 4: gz from backward_params is bit-equal to backward_input's (both
    plans), and a sample of parameter gradients against float64: the first and last conv, the transposed conv of block 2, one
    ResidualUnit per stage, with all their alpha / g / bias."""
    from multimodal_vqvae_compression_audio_tactile_amd import Decoder, synth
    sd = synth.decoder_state(74)
    dec = Decoder(); dec.load_state_dict(sd, strict=True); dec = dec.to(dev)
    sample = ["model.0", "model.2.block.0", "model.2.block.1", "model.1.block.2.block", "model.2.block.3.block", "model.3.block.4.block",
              "model.4.block.2.block", "model.5", "model.6"]
    names = [n for n, _ in dec.named_parameters() if any(n.startswith(s + ".") for s in sample)]
    assert len(names) == 3 + 1 + 3 + 4 * 8 + 1 + 3
    for n, p in dec.named_parameters():
        p.requires_grad_(n in names)
    gen = torch.Generator().manual_seed(74)
    z = 0.3 * torch.randn(1, 1024, 4, generator=gen)
    gy = torch.randn(1, 1, fc.out_len(4, (8, 5, 4, 2)), generator=gen)
    (ref64, _), (ref32, _) = _oracle_grads(sd, z, gy, {})
    zd, gd = z.to(dev), gy.to(dev)
    _, saved = dec._forward_saving_plan(zd)
    saved["z"] = zd
    gz, grads = dec.backward_params(saved, gd)
    assert sorted(grads) == sorted(names)
    _, saved_stack = dec.forward_saving(zd)                                      # the product's plan for a frozen decoder (the stack blob)
    assert torch.equal(gz, dec.backward_input(saved_stack, gd))
    _check_param_grads(grads, ref64, ref32, names, "full")
    _report()


def _backward_profile(dec, z, gy):
    from multimodal_vqvae_compression_audio_tactile_amd import ops
    zr = z.clone().requires_grad_(True)
    with torch.enable_grad():
        y = dec(zr)
    ops.profile_begin()
    try:
        y.backward(gy)
    finally:
        prof = ops.profile_end()
    return zr.grad, {k: v["launches"] for k, v in prof.items()}


def test_subset_trainable_and_frozen_launch_sequences(small, dev):
    """Only the last DecoderBlock trainable: frozen parameters keep grad None and the profile shows weight-gradient, Snake-backward
    and bias launches for that block's 7 convs / 7 Snakes alone.  All frozen: dec(z) under autograd launches exactly what
    Decoder.backward_input launches (the parent's path), kernel for kernel."""
    from multimodal_vqvae_compression_audio_tactile_amd import ops
    _, dec = small
    gen = torch.Generator().manual_seed(9)
    z = (0.5 * torch.randn(2, fc.SMALL["input_channel"], 7, generator=gen)).to(dev)
    gy = torch.randn(2, 1, fc.out_len(7, fc.SMALL["rates"]), generator=gen).to(dev)
    for p in dec.parameters():
        p.requires_grad_(False); p.grad = None
    gz_frozen, frozen = _backward_profile(dec, z, gy)
    _, saved = dec.forward_saving(z)
    ops.profile_begin()
    try:
        gz_direct = dec.backward_input(saved, gy)
    finally:
        direct = {k: v["launches"] for k, v in ops.profile_end().items()}
    assert frozen == direct and torch.equal(gz_frozen, gz_direct), (frozen, direct)
    assert not any("wgrad" in k or "snake_bwd" in k or "bias_grad" in k for k in frozen), frozen
    for n, p in dec.named_parameters():
        p.requires_grad_(n.startswith("model.2."))
    gz_sub, sub = _backward_profile(dec, z, gy)
    assert torch.equal(gz_sub, gz_frozen)
    for n, p in dec.named_parameters():
        assert (p.grad is not None) == n.startswith("model.2."), n
        assert p.grad is None or bool(torch.isfinite(p.grad).all()), n
    count = lambda key: sum(v for k, v in sub.items() if key in k)
    assert count("wgrad") == 7 and count("snake_bwd") == 7 and count("bias_grad") == 7, sub
    for p in dec.parameters():
        p.requires_grad_(False); p.grad = None


def test_second_backward_raises_and_memory_is_released(small, dev):
    """The trainable path keeps _DecoderInputGrad's release-once behaviour: a second backward raises the same error, and with the
    cyclic collector off the allocated memory after steps 1, 2 and 3 is equal (no cycle through the autograd node)."""
    _, dec = small
    for p in dec.parameters():
        p.requires_grad_(True); p.grad = None
    z = (0.3 * torch.randn(4, fc.SMALL["input_channel"], 20, generator=torch.Generator().manual_seed(3))).to(dev).requires_grad_(True)
    with torch.enable_grad():
        y = dec(z)
        y.sum().backward(retain_graph=True)
        with pytest.raises(RuntimeError, match="backward called twice"):
            y.sum().backward()
    del y
    gc.collect()
    gc.disable()
    try:
        used = []
        for _ in range(3):
            with torch.enable_grad():
                y = dec(z)
                y.sum().backward()
            del y
            z.grad = None
            for p in dec.parameters():
                p.grad = None
            torch.cuda.synchronize()
            used.append(torch.cuda.memory_allocated())
    finally:
        gc.enable()
    assert used[2] == used[1] == used[0], used
    for p in dec.parameters():
        p.requires_grad_(False)


def test_arith_modes_refuse_a_trainable_decoder(small, dev):
    from multimodal_vqvae_compression_audio_tactile_amd import ops
    from multimodal_vqvae_compression_audio_tactile_amd._lib import MvqError
    _, dec = small
    z = torch.zeros(1, fc.SMALL["input_channel"], 4, device=dev)
    dec.model[0].bias.requires_grad_(True)
    try:
        for mode in ("bf16x6", "f16x3"):
            with ops.arith(mode), torch.enable_grad(), pytest.raises(MvqError, match="trainable decoder runs in the 'f32' arithmetic only"):
                dec(z)
        assert ops.get_arith() == "f32"
    finally:
        dec.model[0].bias.requires_grad_(False)


# ------------------------------------------------------------------------------------------------------------------ the training step
def _loss(out, wy):
    y, tgt = out["y_hat"], out["tgt"]
    return (y - tgt).abs().mean() + (y * wy[..., :y.shape[-1]]).mean()


@pytest.mark.parametrize("link", [False, True], ids=["default", "link"])
def test_forward_step_trains_the_decoder_and_leaves_the_head_gradients(link, dev):
    """AllPredAR.forward_step at B = 2 with train.unfreeze_decoder: the 21 head tensors get bit for bit the gradients of the
    frozen-decoder step (gz keeps its bits), every decoder parameter a finite gradient; once more under nb_valid / na_valid /
    audio_conceal="mask"."""
    from multimodal_vqvae_compression_audio_tactile_amd import AllPredAR, build_proposed, synth, train
    sd = synth.proposed_model_state(23, rvq_books=3, rvq_embed=128)
    T = 320 * 12
    a = synth.audio_segments(2, seed=9, T=T).to(dev); t = synth.tactile_segments(2, seed=9, T=T).to(dev)
    wy = (0.05 * torch.randn(2, 1, T, generator=torch.Generator().manual_seed(4))).to(dev)
    net = build_proposed(sd, rvq_books=3, rvq_embed=128, device=dev, cls=AllPredAR)
    kw = {}
    if link:
        gen = torch.Generator().manual_seed(12)
        kw = dict(nb_valid=torch.randint(0, 4, (2, 12), generator=gen).to(torch.uint8).to(dev),
                  na_valid=torch.randint(0, 33, (2, 12), generator=gen).to(torch.uint8).to(dev), audio_conceal="mask")
    with torch.enable_grad():
        _loss(net.forward_step(a, t, **kw), wy).backward()
    head = {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}
    assert len(head) == 21 and not any(n.startswith("T_DEC.") for n in head)
    net.zero_grad(set_to_none=True)
    ps = train.unfreeze_decoder(net)
    assert len(ps) == len(list(net.T_DEC.parameters()))
    with torch.enable_grad():
        _loss(net.forward_step(a, t, **kw), wy).backward()
    for n, g in head.items():
        assert torch.equal(dict(net.named_parameters())[n].grad, g), n
    for n, p in net.T_DEC.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape and bool(torch.isfinite(p.grad).all()), n
        assert float(p.grad.abs().max()) > 0, n
    # a decoder-only fine-tune: the head frozen, z_run carries no graph
    net.zero_grad(set_to_none=True)
    for n, p in net.named_parameters():
        if not n.startswith("T_DEC."):
            p.requires_grad_(False)
    with torch.enable_grad():
        _loss(net.forward_step(a, t, **kw), wy).backward()
    assert all(p.grad is not None for p in net.T_DEC.parameters())
    assert all(p.grad is None for n, p in net.named_parameters() if not n.startswith("T_DEC."))


def test_optimiser_step_is_seen_by_the_caches_and_matches_torch(small, dev):
    """One optim.AdamW step over the decoder parameters: dec(z) afterwards equals a fresh Decoder loaded from the updated
    state_dict() (the packed / folded weight caches saw the in-place step), and the parameters match torch.optim.AdamW on the same
    gradients within rtol 1e-6, atol 1e-7."""
    from multimodal_vqvae_compression_audio_tactile_amd import Decoder, optim, train
    sd, dec = small
    dec.load_state_dict(sd, strict=True)
    ps = train.unfreeze_decoder(dec)
    z, tgt = (x.to(dev) for x in fc.learn_batch())
    with torch.enable_grad():
        y0 = dec(z).detach()                                                     # fills every packed-weight cache before the step
    for p in ps:
        p.grad = None
    with torch.enable_grad():
        (dec(z) - tgt).abs().mean().backward()
    twin = [torch.nn.Parameter(p.detach().cpu().clone()) for p in ps]
    for q, p in zip(twin, ps):
        q.grad = p.grad.detach().cpu().clone()
    optim.clip_grad_norm_(ps, 1e9)                                               # takes the new parameters like any others (no-op clip)
    opt = optim.AdamW(ps, lr=1e-3)
    opt.step()
    torch.optim.AdamW(twin, lr=1e-3).step()
    for (n, _), p, q in zip(dec.trainable(), ps, twin):
        assert torch.allclose(p.detach().cpu(), q.detach(), rtol=1e-6, atol=1e-7), n
    fresh = Decoder(**fc.SMALL)
    fresh.load_state_dict(dec.state_dict(), strict=True)
    fresh = fresh.to(dev)
    train.unfreeze_decoder(fresh)
    with torch.enable_grad():                                                    # (this small shape has no one-call inference stack)
        y1, y2 = dec(z).detach(), fresh(z).detach()
    assert torch.equal(y1, y2) and not torch.equal(y1, y0)
    dec.load_state_dict(sd, strict=True)
    for p in dec.parameters():
        p.requires_grad_(False); p.grad = None


def test_five_adamw_steps_learn(small, dev):
    """The fixed batch and learning rate of decoder_finetune_cases.LEARN (on which the float64 restatement decreases strictly,
    tests/test_decoder_finetune_cpu.py): five optim.AdamW steps on the L1 loss end strictly below the first loss.  The restatement's
    losses are printed beside them (Adam's first steps are +-lr whatever the gradient's size, so no bound ties the two curves)."""
    from multimodal_vqvae_compression_audio_tactile_amd import optim, train
    sd, dec = small
    dec.load_state_dict(sd, strict=True)
    ps = train.unfreeze_decoder(dec)
    for p in ps:
        p.grad = None
    z, tgt = (x.to(dev) for x in fc.learn_batch())
    opt = optim.AdamW(ps, lr=fc.LEARN["lr"])
    losses = []
    for _ in range(fc.LEARN["steps"]):
        opt.zero_grad(set_to_none=True)
        with torch.enable_grad():
            loss = (dec(z) - tgt).abs().mean()
            loss.backward()
        losses.append(float(loss.detach()))
        opt.step()
    with torch.enable_grad():
        losses.append(float((dec(z) - tgt).abs().mean().detach()))
    want = fc.learn_oracle()
    print("HIP", losses, "float64", want)
    assert want[-1] < want[0] and losses[-1] < losses[0]
    dec.load_state_dict(sd, strict=True)
    for p in dec.parameters():
        p.requires_grad_(False); p.grad = None
