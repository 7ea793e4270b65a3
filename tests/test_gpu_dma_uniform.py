"""-m gpu: the uniform-advance LDS-DMA K loop (csrc/conv1d_mfma.hpp) against the CPU oracle, BIT-EXACT.

Interior tiles stage their chunks from a scalar base + a constant per-lane offset and walk the ring in a loop unrolled by its
three stages; edge tiles (a piece outside its row), virtually packed rows and rows that are not 16-byte multiples keep the earlier
forms.  Every case names the kernel instantiation it must run -- asked of the dispatcher in name mode (the launchers' name_out)
and checked against what the launch profiler saw -- so that a case cannot pass on another kernel.  Shapes are the smallest for which
the dispatcher's own rule picks the family: >= 4 column tiles (both edge tiles and interior ones), and input-channel counts whose
chunk counts are 0, 1 and 2 mod 3 (the unrolled loop's remainders), one case with two chunks only."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _rng(*seed):
    """Generator seeded by a tuple of integers (the same data in every process)."""
    return np.random.default_rng([int(v) for v in seed])


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


class _ran:
    """with _ran(name): ... -- the block launched exactly that kernel instantiation (launch profiler)."""

    def __init__(self, *names):
        self.names = set(names)

    def __enter__(self):
        from multimodal_vqvae_compression_audio_tactile_amd import ops
        ops.profile_begin()
        return self

    def __exit__(self, et, ev, tb):
        from multimodal_vqvae_compression_audio_tactile_amd import ops
        prof = ops.profile_end()
        if et is None:
            assert set(prof) == self.names, (sorted(prof), sorted(self.names))
        return False


K7 = "conv1d_mfma_kernel<7, 1, %d, %s, 0>"
T128, T96, T64 = "4, 2, 2, 2, 2", "4, 3, 1, 1, 4", "8, 1, 1, 2, 2"     # CK, MT, NT, WAVES_M, WAVES_N of the three families
# (B, Cin, T, Cout, dil, tile): chunks = Cin / CK
K7_CASES = [
    (4, 192, 7168, 128, 1, T128),      # 48 chunks (0 mod 3), 224 tiles of 128 x 128
    (4, 160, 7168, 128, 3, T128),      # 40 (1 mod 3)
    (4, 128, 7168, 128, 9, T128),      # 32 (2 mod 3)
    (2, 192, 1408, 96, 3, T96),        # 96-row tile: 672 weight pieces = 10.5 wave-instructions, re-dealt; 11 column tiles (fewer
    (2, 160, 1408, 96, 9, T96),        # 16 x 16 tiles than this and the dispatcher takes the one-wave latency kernel instead)
    (2, 128, 1408, 96, 1, T96),
    (1, 192, 2064, 128, 9, T64),       # 64 x 64 tiles (a grid that cannot fill the chip with 128-row tiles): 24 chunks of 8
    (1, 128, 2064, 128, 1, T64),       # 16 (1 mod 3); the last of the 33 column tiles is a quarter full
    (1, 160, 2064, 128, 3, T64),       # 20 (2 mod 3)
]


def _k7(case, orc, dev, tin=None):
    from multimodal_vqvae_compression_audio_tactile_amd import ops
    B, Cin, T, Cout, dil, tile = case
    T = tin or T
    name = K7 % (dil, tile)
    assert ops.conv_kernel_name(Cin, Cout, 7, 1, dil, tin=T, batch=B) == name
    r = _rng(*case[:5], T)
    x = r.standard_normal((B, Cin, T)).astype(np.float32)
    w = (r.standard_normal((Cout, Cin, 7)) / math.sqrt(Cin * 7)).astype(np.float32)
    b = (0.1 * r.standard_normal(Cout)).astype(np.float32)
    ao = r.uniform(0.5, 1.5, Cout).astype(np.float32)
    want = orc.conv1d(x, w, b, 1, dil, 3 * dil, None, None, ao, False)
    wp = ops.pack_conv1d(_t(w, dev))
    with _ran(name):
        got = ops.conv1d(_t(x, dev), wp, Cout, 7, bias=_t(b, dev), dil=dil, pad=3 * dil, alpha_out=_t(ao, dev))
    got = got.cpu().numpy()
    assert got.shape == want.shape and np.array_equal(got, want), f"max abs diff {np.abs(got - want).max()}"


@pytest.mark.parametrize("case", K7_CASES, ids=[f"k7_{c[5].split(', ')[1]}{c[5].split(', ')[2]}_c{c[1]}_d{c[4]}" for c in K7_CASES])
def test_seven_tap_uniform_loop_bit_exact(case, orc, dev):
    _k7(case, orc, dev)


def test_row_length_not_a_multiple_of_four_keeps_the_register_staged_loop(orc, dev):
    """Rows that are not 16-byte multiples cannot be staged by LDS-DMA at all: same instantiation, register-staged K loop."""
    _k7((4, 128, 7168, 128, 3, T128), orc, dev, tin=7170)


# 1x1 conv with skip and dual Snake output (the second conv of a wide ResidualUnit): (B, Cin, T, Cout, kernel)
K1_CASES = [
    (4, 192, 3584, 192, "conv1d_mfma_kernel<1, 1, 1, 16, 3, 1, 1, 4, 0>"),     # 96-row tile (384 weight pieces: six full instructions), 12 chunks
    (4, 256, 3584, 256, "conv1d_mfma_kernel<1, 1, 1, 16, 2, 2, 2, 2, 0>"),     # 128-row tile, 16 chunks (1 mod 3)
    (8, 32, 3584, 128, "conv1d_mfma_kernel<1, 1, 1, 16, 2, 2, 2, 2, 0>"),      # two chunks only: nothing but the peeled end
]


@pytest.mark.parametrize("case", K1_CASES, ids=[f"k1_c{c[1]}_m{c[3]}" for c in K1_CASES])
def test_one_by_one_with_skip_and_dual_output_bit_exact(case, orc, dev):
    from multimodal_vqvae_compression_audio_tactile_amd import ops
    B, Cin, T, Cout, name = case
    assert ops.conv_kernel_name(Cin, Cout, 1, tin=T, batch=B) == name
    r = _rng(*case[:4])
    x = r.standard_normal((B, Cin, T)).astype(np.float32)
    w = (r.standard_normal((Cout, Cin, 1)) / math.sqrt(Cin)).astype(np.float32)
    b = (0.1 * r.standard_normal(Cout)).astype(np.float32)
    res = r.standard_normal((B, Cout, T)).astype(np.float32)
    a2 = r.uniform(0.5, 1.5, Cout).astype(np.float32)
    want = orc.conv1d(x, w, b, 1, 1, 0, None, res, None, False)
    with _ran(name):
        y, y2 = ops.conv1d(_t(x, dev), ops.pack_conv1d(_t(w, dev)), Cout, 1, bias=_t(b, dev), residual=_t(res, dev), alpha_dual=_t(a2, dev))
    assert np.array_equal(y.cpu().numpy(), want)
    assert np.array_equal(y2.cpu().numpy(), orc.snake(want, a2))


# (C, dil, B, T, kernel): the dispatcher's name mode answers for the throughput form (at least 200 blocks of 128 columns); a smaller
# grid at C = 128 takes the half-width tile
RU_CASES = [
    (96, 3, 2, 600, None),
    (128, 1, 8, 3200, None),
    (128, 9, 2, 600, "residual_unit_kernel<9, 4, 2, 1, 2, 2>"),
]


@pytest.mark.parametrize("C,dil,B,T,name", RU_CASES, ids=[f"ru{c[0]}_d{c[1]}_b{c[2]}" for c in RU_CASES])
def test_fused_unit_on_presnaked_input_bit_exact(C, dil, B, T, name, orc, dev):
    """The one-launch ResidualUnit fed with snake_a(x) (its 7-tap stage then runs on the LDS-DMA ring) == the two oracle convs."""
    from multimodal_vqvae_compression_audio_tactile_amd import ops
    name = name or ops.residual_unit_kernel_name(C, dil)
    assert name.startswith(f"residual_unit_kernel<{dil}, 4, ")
    r = _rng(C, dil)
    x = r.standard_normal((B, C, T)).astype(np.float32)
    w7 = (r.standard_normal((C, C, 7)) / math.sqrt(C * 7)).astype(np.float32)
    w1 = (r.standard_normal((C, C, 1)) / math.sqrt(C)).astype(np.float32)
    b7 = (0.1 * r.standard_normal(C)).astype(np.float32); b1 = (0.1 * r.standard_normal(C)).astype(np.float32)
    aa, ab, an = (r.uniform(0.5, 1.5, C).astype(np.float32) for _ in range(3))
    h = orc.conv1d(x, w7, b7, dil=dil, pad=3 * dil, alpha_in=aa)
    want = orc.conv1d(h, w1, b1, alpha_in=ab, residual=x, alpha_out=an)
    xs = _t(orc.snake(x, aa), dev)
    w7p, w1p = ops.pack_conv1d(_t(w7, dev)), ops.pack_conv1d(_t(w1, dev))
    with _ran(name):
        got = ops.residual_unit(_t(x, dev), w7p, _t(b7, dev), _t(aa, dev), _t(ab, dev), w1p, _t(b1, dev), dil, alpha_next=_t(an, dev), x_snaked=xs)
    assert np.array_equal(got.cpu().numpy(), want), f"max abs diff {np.abs(got.cpu().numpy() - want).max()}"


def test_strided_conv_bit_exact(orc, dev):
    from multimodal_vqvae_compression_audio_tactile_amd import ops
    B, Cin, T, Cout, s = 4, 64, 35840, 128, 5                  # 224 tiles of 128 x 128, 32 chunks of 2 channels
    name = "conv1d_mfma_kernel<10, 5, 1, 2, 2, 2, 2, 2, 0>"
    assert ops.conv_kernel_name(Cin, Cout, 2 * s, s, tin=T, batch=B) == name
    r = _rng(B, Cin, T, Cout, s)
    x = r.standard_normal((B, Cin, T)).astype(np.float32)
    w = (r.standard_normal((Cout, Cin, 2 * s)) / math.sqrt(Cin * 2 * s)).astype(np.float32)
    b = (0.1 * r.standard_normal(Cout)).astype(np.float32)
    want = orc.conv1d(x, w, b, s, 1, 3, None, None, None, False)
    with _ran(name):
        got = ops.conv1d(_t(x, dev), ops.pack_conv1d(_t(w, dev)), Cout, 2 * s, bias=_t(b, dev), stride=s, pad=3)
    assert np.array_equal(got.cpu().numpy(), want)


def test_transposed_conv_bit_exact(orc, dev):
    from multimodal_vqvae_compression_audio_tactile_amd import ops
    B, Cin, T, Cout, s = 8, 64, 1792, 64, 4                     # 256 GEMM rows (4 phases), 240 tiles of 128 x 128
    name = ops.conv_kernel_name(Cin, Cout, 2 * s, s, transposed=True, tin=T, batch=B)
    assert name == "conv1d_mfma_kernel<2, 1, 1, 8, 2, 2, 2, 2, 4>"
    r = _rng(B, Cin, T, Cout, s, 1)
    x = r.standard_normal((B, Cin, T)).astype(np.float32)
    w = (r.standard_normal((Cin, Cout, 2 * s)) / math.sqrt(Cin * 2)).astype(np.float32)
    b = (0.1 * r.standard_normal(Cout)).astype(np.float32)
    want = orc.conv_transpose1d(x, w, b, s, 2, None, None)
    with _ran(name):
        got = ops.conv_transpose1d(_t(x, dev), ops.pack_conv_transpose1d(_t(w, dev), s), Cout, s, 2, bias=_t(b, dev))
    assert np.array_equal(got.cpu().numpy(), want)


def test_virtually_packed_call_equals_its_plain_form(dev):
    """Virtually packed rows remap every piece per lane: the block keeps the per-lane pointers, and equals the plain launch (whose
    interior tiles take the uniform form)."""
    from multimodal_vqvae_compression_audio_tactile_amd import ops
    g = torch.Generator().manual_seed(5)
    r = lambda *s: torch.randn(*s, generator=g).to(dev)
    B = 13
    x, w, bias = r(B, 128, 600), r(256, 128, 16) / 45.0, r(256)
    wp = ops.pack_conv1d(w)
    want = ops.conv1d(x, wp, 256, 16, bias=bias, stride=8, pad=4)
    tout, rows, per_in = ops.vpacked_geometry(600, 600, 16, 8, 1, 4, follow_pad=1)
    ops.profile_begin()
    try:
        got = ops.conv1d_vpacked(x, wp, 256, 16, 10, 600, rows, bias=bias, stride=8, pad=4)
    finally:
        prof = ops.profile_end()
    assert list(prof) == ["conv1d_mfma_kernel<16, 8, 1, 1, 2, 2, 2, 2, 0>"], prof
    assert torch.equal(got[..., :tout], want) and not got[..., tout:].any()
