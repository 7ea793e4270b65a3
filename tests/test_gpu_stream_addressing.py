"""-m gpu: the two instantiations of each streaming state kernel against each other -- the slot addressing of a pool group and
the dense addressing of a lockstep session run ONE kernel body (csrc/stream.hip), so the same data gives the same bits.  C = 40
is no multiple of the window kernel's 32-row block: the 80 rows of the group [2, 0] make three blocks, the second spans the
session boundary at row 40 (two slots in one block) and the third holds 16 rows.  Every comparison is an equality."""
import pytest
import torch

pytestmark = pytest.mark.gpu

S_POOL, SLOTS, C = 3, [2, 0], 40


def test_window_slots_equal_the_dense_window_across_a_session_boundary(dev):
    from multimodal_vqvae_compression_audio_tactile_amd import ops
    g = torch.Generator().manual_seed(40)
    pool = torch.randn(S_POOL, C, 20, generator=g).to(dev)
    dense = pool[SLOTS].clone()
    other = pool[1].clone()
    for h_in, n, h_out in [(0, 16, 16), (16, 16, 20), (20, 16, 20), (20, 5, 20)]:
        z = torch.randn(len(SLOTS), C, n, generator=g).to(dev)
        win_pool = ops.stream_window_slots(pool, SLOTS, h_in, z, h_out)
        win_dense = ops.stream_window(dense, h_in, z, h_out)
        assert win_pool.shape == (len(SLOTS), C, h_in + n)
        assert torch.equal(win_pool, win_dense), (h_in, n, h_out)
        assert torch.equal(win_dense[..., h_in:], z)
        assert torch.equal(pool[SLOTS], dense), (h_in, n, h_out)
        assert torch.equal(pool[1], other), (h_in, n, h_out)                    # the unlisted slot: bit for bit what it was


def test_resampler_slots_equal_the_dense_resampler(dev):
    from multimodal_vqvae_compression_audio_tactile_amd import ops
    from multimodal_vqvae_compression_audio_tactile_amd.resample import sinc_resample_kernel
    kern, width, orig, new = sinc_resample_kernel(24000, 3000)
    kern = kern.to(dev)
    pool = ops.resample_stream_state(orig, width, S_POOL, dev)
    dense = ops.resample_stream_state(orig, width, len(SLOTS), dev)
    pieces = [1920, 5120, 5120, 1592]
    x = torch.randn(len(SLOTS), sum(pieces), generator=torch.Generator().manual_seed(3000)).to(dev)
    pos = 0
    for i, n in enumerate(pieces):
        final = i == len(pieces) - 1
        y_pool = ops.resample_stream_slots(x[:, pos:pos + n], kern, pool, SLOTS, pos, orig, new, width, final=final)
        y_dense = ops.resample_stream(x[:, pos:pos + n], kern, dense, pos, orig, new, width, final=final)
        assert y_pool.shape == (len(SLOTS), ops.resample_stream_out_len(pos, n, orig, width, final)) and y_pool.shape[1] > 0
        assert torch.equal(y_pool, y_dense), i
        assert torch.equal(pool[SLOTS], dense), i
        assert not pool[1].any(), i                                             # the unlisted slot's state stays zero
        pos += n
