"""-m gpu: the decoder's input-gradient (mvq_conv1d_dgrad_f32 on flipped / transposed weight images, Snake derivative and skip
gradient fused into the epilogue) BIT-EXACT against the C oracle, one case per kernel form the training step launches.

DGRAD_CASES holds one small case per (instantiation, epilogue): the latency forms, the 64 x 64 / 96-row / 128 x 96 tiles, the
column-split tail launches (conv_tail_width) and the direct Cin = 1 kernel, with lengths that are not a multiple of 4 and with
operands one float past a 16-byte boundary.  test_dgrad_cases_cover_the_decoder_backward profiles Decoder.backward_input at the
reference's training batch (6) and at bench.py's (256) and fails, naming the instantiation, when the dispatch launches a form
that no case here checks.  The full-size decoder input-gradient is then tied to the oracle at those batches."""
import math
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _np(sd):
    return {k: v.numpy() for k, v in sd.items()}


# (B, Cin, Tin, Cout, ks, stride, dil, epilogue, misaligned, tiny_alpha) in FORWARD geometry: the layer maps x[B, Cin, Tin] to
# y[B, Cout, Tout] and the case computes gx[B, Cin, Tin] from gy[B, Cout, Tout].  stride 1: Conv1d(ks, dil, pad = 3 dil)
# (Tout = Tin); stride s > 1: the DecoderBlock ConvTranspose1d (kernel 2 s, pad ceil(s / 2)), whose input-gradient is a strided conv.
# epilogue: "none" (model.0), "dsnake" (gx * Snake'(x): the 1x1 convs, the up-sampling convs, the last conv), "dsnake+res"
# (+ the skip gradient: the 7-tap convs).  misaligned: gy, the Snake source and the residual start one float past a 16-byte
# boundary (no 16-byte loads, no LDS-DMA staging, no 16-byte stores).  tiny_alpha: some channels get alpha ~ 1e-3, where the
# 1 / (alpha + 1e-9) of the derivative matters.  Channel counts are cut to what the dispatch needs to pick the same form.
DGRAD_CASES = [
    # latent rate (75 frames): model.0 and the first DecoderBlock's up-sampling conv
    (2, 1024, 75, 256, 7, 1, 1, "none", False, False),         # conv1d_lat_kernel<7, 1, 1, 16>            (B = 6)
    (64, 512, 75, 64, 7, 1, 1, "none", False, False),          # mfma<7, 1, 1, 4, 1, 3, 4, 1>: 128 x 96 tile (B = 256)
    (64, 512, 75, 64, 7, 1, 1, "none", True, False),
    (2, 256, 75, 64, 16, 8, 1, "dsnake", False, True),         # conv1d_lat_kernel<16, 8, 1, 8>            (B = 6)
    (64, 512, 75, 32, 16, 8, 1, "dsnake", False, False),       # mfma<16, 8, 1, 1, 1, 3, 4, 1>: 128 x 96, LDS-DMA (B = 256)
    (64, 512, 75, 32, 16, 8, 1, "dsnake", True, True),         # mfma<16, 8, 1, 2, 1, 3, 4, 1>: register-staged
    # 600-sample level at B = 6: 64 x 64 tiles
    (2, 256, 600, 64, 1, 1, 1, "dsnake", False, False),        # mfma<1, 1, 1, 32, 1, 1, 2, 2>
    (2, 256, 600, 64, 7, 1, 1, "dsnake+res", False, False),    # mfma<7, 1, D, 8, 1, 1, 2, 2>
    (2, 256, 600, 64, 7, 1, 3, "dsnake+res", True, False),
    (2, 256, 600, 64, 7, 1, 9, "dsnake+res", False, True),
    (2, 256, 600, 64, 10, 5, 1, "dsnake", False, False),       # mfma<10, 5, 1, 4, 1, 1, 2, 2>: gy 2999 samples
    # 600-sample level at B = 256: four 128-column tiles + a 96-column tail launch (B x row tiles >= 128)
    (128, 128, 600, 64, 1, 1, 1, "dsnake", False, False),      # mfma<1, 1, 1, 16, 2, 2, 2, 2> + <1, 1, 1, 16, 1, 3, 4, 1>
    (128, 128, 216, 64, 1, 1, 1, "dsnake", True, True),
    (128, 128, 216, 32, 7, 1, 1, "dsnake+res", False, False),  # mfma<7, 1, D, 4, 2, 2, 2, 2> + <7, 1, D, 4, 1, 3, 4, 1>
    (128, 128, 600, 32, 7, 1, 3, "dsnake+res", False, True),
    (128, 128, 216, 32, 7, 1, 9, "dsnake+res", True, False),
    (128, 128, 216, 32, 10, 5, 1, "dsnake", False, False),     # mfma<10, 5, 1, 2, 2, 2, 2, 2> + <10, 5, 1, 2, 1, 3, 4, 1>
    (128, 128, 216, 32, 10, 5, 1, "dsnake", True, True),
    # 2999-sample level at B = 256: 128-column tiles + a 64-column tail launch; odd lengths (scalar staging and stores)
    (128, 128, 183, 64, 1, 1, 1, "dsnake", False, False),      # mfma<1, 1, 1, 16, 2, 2, 2, 2> + <1, 1, 1, 16, 2, 1, 2, 2>
    (128, 128, 183, 32, 7, 1, 1, "dsnake+res", False, True),   # mfma<7, 1, D, 4, 2, 2, 2, 2> + <7, 1, D, 4, 2, 1, 2, 2>
    (128, 128, 183, 32, 7, 1, 3, "dsnake+res", True, False),
    (128, 128, 183, 32, 7, 1, 9, "dsnake+res", False, False),
    (128, 128, 183, 32, 8, 4, 1, "dsnake", False, False),      # mfma<8, 4, 1, 2, 2, 2, 2, 2> + <8, 4, 1, 2, 2, 1, 2, 2>
    (128, 128, 183, 32, 8, 4, 1, "dsnake", True, True),        # mfma<8, 4, 1, 4, 2, 2, 2, 2> (register-staged) + the tail
    (128, 128, 216, 32, 8, 4, 1, "dsnake", False, False),      # mfma<8, 4, 1, 2, 1, 3, 4, 1>: the 96-column tail of s = 4
    (128, 128, 183, 32, 10, 5, 1, "dsnake", False, False),     # mfma<10, 5, 1, 2, 2, 1, 2, 2>: the 64-column tail of s = 5
    # 2999-sample level at B = 6: 128 x 128 tiles, no split (the tail launch could not fill the chip)
    (6, 384, 2999, 64, 1, 1, 1, "dsnake", False, False),       # mfma<1, 1, 1, 16, 2, 2, 2, 2>
    (3, 384, 2999, 32, 7, 1, 3, "dsnake+res", False, True),    # mfma<7, 1, 3, 4, 2, 2, 2, 2>
    (3, 384, 2999, 32, 7, 1, 9, "dsnake+res", True, False),
    (3, 384, 2999, 32, 7, 1, 1, "dsnake+res", False, False),
    (3, 384, 2999, 32, 8, 4, 1, "dsnake", False, False),       # mfma<8, 4, 1, 2, 2, 2, 2, 2>: gy 11 996 samples
    # 11 996 / 23 992-sample levels (192 / 96 channels): 96-row tiles
    (4, 192, 6001, 64, 1, 1, 1, "dsnake", False, False),       # mfma<1, 1, 1, 16, 3, 1, 1, 4>
    (4, 96, 6501, 64, 1, 1, 1, "dsnake", True, True),
    (2, 192, 1001, 64, 7, 1, 1, "dsnake+res", False, False),   # mfma<7, 1, D, 4, 3, 1, 1, 4>
    (2, 192, 1000, 64, 7, 1, 3, "dsnake+res", False, True),
    (4, 96, 6000, 32, 7, 1, 3, "dsnake+res", False, False),
    (2, 192, 1001, 64, 7, 1, 9, "dsnake+res", True, False),
    (2, 192, 1000, 96, 4, 2, 1, "dsnake", False, False),       # mfma<4, 2, 1, 4, 3, 1, 1, 4>: LDS-DMA
    (2, 192, 1001, 96, 4, 2, 1, "dsnake", True, True),         # mfma<4, 2, 1, 8, 3, 1, 1, 4>
    # the last conv (96 -> 1 channel): its input-gradient runs the direct Cin = 1 kernel
    (2, 96, 2999, 1, 7, 1, 1, "dsnake", False, True),          # conv1d_cin1_kernel<7>
    (2, 96, 2000, 1, 7, 1, 1, "dsnake", True, False),
    # latency forms at one segment (one wave per 16 x 16 tile)
    (1, 256, 75, 128, 1, 1, 1, "dsnake", False, False),        # conv1d_lat_kernel<1, 1, 1, 64>
    (1, 256, 150, 64, 7, 1, 1, "dsnake+res", False, True),     # conv1d_lat_kernel<7, 1, D, 16>
    (1, 256, 150, 64, 7, 1, 3, "dsnake+res", True, False),
    (1, 256, 150, 64, 7, 1, 9, "dsnake+res", False, False),
    (1, 256, 75, 64, 10, 5, 1, "dsnake", False, True),         # conv1d_lat_kernel<10, 5, 1, 8>
    (1, 256, 75, 64, 16, 8, 1, "dsnake", True, False),         # conv1d_lat_kernel<16, 8, 1, 8>
]


def _case_id(c):
    B, cin, tin, cout, ks, s, d, epi, mis, tiny = c
    return f"B{B}-{cin}x{tin}-{cout}-k{ks}s{s}d{d}-{epi}" + ("-mis" if mis else "") + ("-tiny" if tiny else "")


def _dev_view(a, dev, misaligned):
    """a on the device; misaligned: as a contiguous view that starts one float past a 16-byte boundary (buf[1:])."""
    if not misaligned:
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    buf = torch.empty(a.size + 1, dtype=torch.float32, device=dev)
    v = buf[1:].view(a.shape)
    v.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    assert v.data_ptr() % 16 == 4
    return v


def _case_inputs(case):
    B, cin, tin, cout, ks, s, d, epi, mis, tiny = case
    r = np.random.default_rng(zlib.crc32(repr(case).encode()))
    if s == 1:
        pad = 3 * d if ks == 7 else (ks - 1) * d // 2
        w = (r.standard_normal((cout, cin, ks)) / math.sqrt(cout * ks)).astype(np.float32)
        tout = tin
    else:
        pad = math.ceil(s / 2)
        w = (r.standard_normal((cin, cout, ks)) / math.sqrt(cout * 2)).astype(np.float32)
        tout = (tin - 1) * s - 2 * pad + ks
    gy = r.standard_normal((B, cout, tout)).astype(np.float32)
    src = alpha = res = None
    if epi != "none":
        src = (2.0 * r.standard_normal((B, cin, tin))).astype(np.float32)
        alpha = r.uniform(0.5, 1.5, cin).astype(np.float32)
        if tiny:
            alpha[r.random(cin) < 0.2] = np.float32(1e-3)
    if epi == "dsnake+res":
        res = r.standard_normal((B, cin, tin)).astype(np.float32)
    return w, gy, src, alpha, res, pad


def _run_case(case, dev, inputs=None):
    from multimodal_vqvae_compression_audio_tactile_amd import ops
    B, cin, tin, cout, ks, s, d, epi, mis, tiny = case
    w, gy, src, alpha, res, pad = inputs if inputs is not None else _case_inputs(case)
    wt = torch.from_numpy(w).to(dev)
    wp = ops.pack_conv1d_dgrad(wt) if s == 1 else ops.pack_conv_transpose1d_dgrad(wt)
    opt = lambda a: None if a is None else _dev_view(a, dev, mis)
    gx = ops.conv1d_dgrad(_dev_view(gy, dev, mis), wp, cin, tin, ks, s, d, pad, dsnake_src=opt(src),
                          dsnake_alpha=None if alpha is None else torch.from_numpy(alpha).to(dev), residual=opt(res))
    torch.cuda.synchronize()
    return gx


@pytest.mark.parametrize("case", DGRAD_CASES, ids=[_case_id(c) for c in DGRAD_CASES])
def test_conv1d_dgrad_bit_exact(case, orc, dev):
    B, cin, tin, cout, ks, s, d, epi, mis, tiny = case
    inputs = _case_inputs(case)
    w, gy, src, alpha, res, pad = inputs
    want = orc.conv1d_dgrad(gy, w, d, pad) if s == 1 else orc.conv_transpose1d_dgrad(gy, w, s, pad)
    if epi != "none":
        want = orc.mul_dsnake(want, src, alpha, residual=res)
    assert want.shape == (B, cin, tin)
    got = _run_case(case, dev, inputs).cpu().numpy()
    assert got.shape == want.shape
    assert np.isfinite(want).all()
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{len(bad)} elements differ, first at {tuple(bad[0])}: max abs diff {np.nanmax(np.abs(got - want))}"


# ------------------------------------------------------------------------------------------------------------------------------
# The decoder's input-gradient at the training batches, tied to the oracle (mirrors test_headline_batch_256_is_tied_to_the_oracle)
T_LAT = 75


@pytest.fixture(scope="module")
def decoder(dev):
    from multimodal_vqvae_compression_audio_tactile_amd import Decoder, synth
    sd = synth.decoder_state(74)
    dec = Decoder(); dec.load_state_dict(sd, strict=True); dec = dec.to(dev)
    for p in dec.parameters():
        p.requires_grad_(False)
    return sd, dec


@pytest.fixture(scope="module")
def oracle_segment(decoder, orc):
    """One full segment (75 latent frames -> 23 992 samples) through the oracle's saving forward and input-gradient."""
    sd, _ = decoder
    g = torch.Generator().manual_seed(75)
    z = 0.3 * torch.randn(1, 1024, T_LAT, generator=g)
    gy = torch.randn(1, 1, 23992, generator=g)
    sdn = _np(sd)
    want_y, saved = orc.dac_decoder_saving(sdn, z.numpy())
    assert want_y.shape == (1, 1, 23992)
    want_gz = orc.dac_decoder_backward_input(sdn, saved, gy.numpy())
    del saved
    return z, gy, want_y, want_gz


def _grad(dec, z, gy, profile=False):
    """dL/dz through autograd (the training step's call site); profile: also the kernel instantiations of the backward."""
    from multimodal_vqvae_compression_audio_tactile_amd import ops
    zr = z.clone().requires_grad_(True)
    with torch.enable_grad():
        y = dec(zr)
    if profile:
        ops.profile_begin()
    y.backward(gy)
    names = set(ops.profile_end()) if profile else None
    torch.cuda.synchronize()
    return zr.grad, names


def _planted(B):
    return (0, B // 2, B - 1)


@pytest.fixture(scope="module")
def decoder_backward_runs(decoder, oracle_segment, dev):
    """Decoder.backward_input at B = 6 and 256 (the stack) and at B = 6 (the Python plan), the oracle's segment planted at the
    first, a middle and the last row: {(B, plan): (rows of z.grad, kernel instantiations launched by the backward)}."""
    from multimodal_vqvae_compression_audio_tactile_amd import dac
    _, dec = decoder
    z1, gy1, _, _ = oracle_segment
    out = {}
    for B, stacks in ((6, True), (6, False), (256, True)):
        g = torch.Generator().manual_seed(B)
        z = 0.3 * torch.randn(B, 1024, T_LAT, generator=g)
        gy = torch.randn(B, 1, 23992, generator=g)
        for i in _planted(B):
            z[i], gy[i] = z1[0], gy1[0]
        z, gy = z.to(dev), gy.to(dev)
        old = dac.USE_STACKS
        dac.USE_STACKS = stacks
        try:
            gz, names = _grad(dec, z, gy, profile=True)
            others = {i: _grad(dec, z[i:i + 1], gy[i:i + 1])[0].cpu() for i in (1, B // 2 + 1, B - 2)}
        finally:
            dac.USE_STACKS = old
        rows = {i: gz[i:i + 1].cpu() for i in set(_planted(B)) | set(others)}
        out[(B, stacks)] = (rows, others, names)
        del gz, z, gy
        torch.cuda.empty_cache()
    return out


def test_decoder_input_gradient_one_segment_bit_exact(decoder, oracle_segment, dev):
    """B = 1, T = 75: dec(z).backward(gy) through autograd == the oracle, bit for bit (and the saving forward's y too)."""
    _, dec = decoder
    z, gy, want_y, want_gz = oracle_segment
    zr = z.to(dev).requires_grad_(True)
    with torch.enable_grad():
        y = dec(zr)
    assert np.array_equal(y.detach().cpu().numpy(), want_y)
    y.backward(gy.to(dev))
    assert np.array_equal(zr.grad.cpu().numpy(), want_gz)


@pytest.mark.parametrize("B,stacks", [(6, True), (6, False), (256, True)], ids=["B6-stack", "B6-plan", "B256-stack"])
def test_decoder_input_gradient_at_training_batches(B, stacks, decoder_backward_runs, oracle_segment):
    """Rows of the B-segment batch that hold the oracle's segment carry the oracle's dL/dz bit for bit, wherever they sit; other
    rows equal their own B = 1 run (batch mates and the batch-dependent launch plan change nothing)."""
    rows, others, _ = decoder_backward_runs[(B, stacks)]
    want = oracle_segment[3]
    for i in _planted(B):
        got = rows[i].numpy()
        assert np.array_equal(got, want), f"row {i} of the {B}-segment batch: max abs diff {np.abs(got - want).max()}"
    for i, g1 in others.items():
        assert torch.equal(rows[i], g1), f"row {i} of the {B}-segment batch differs from its own B = 1 run"


def test_dgrad_cases_cover_the_decoder_backward(decoder_backward_runs, dev):
    """Every kernel instantiation (tail launches included) that Decoder.backward_input launches at B = 6 and B = 256 is one that a
    DGRAD_CASES entry checks against the oracle.  A dispatch change that moves the decoder onto an unchecked form fails here."""
    from multimodal_vqvae_compression_audio_tactile_amd import ops
    ops.profile_begin()
    try:
        for case in DGRAD_CASES:
            _run_case(case, dev)
    finally:
        checked = set(ops.profile_end())
    assert len(checked) >= 30, sorted(checked)
    for (B, stacks), (_, _, launched) in decoder_backward_runs.items():
        assert len(launched) >= 10, (B, stacks, sorted(launched))
        missing = sorted(launched - checked)
        assert not missing, f"decoder backward at B = {B} ({'stack' if stacks else 'Python plan'}) launches instantiations " \
                            f"no DGRAD_CASES entry checks: {missing}"
