"""No GPU: the host side of decoder fine-tuning -- the exports and their refusals (every refusal happens before a launch, so it
can be provoked without a device), the split-K workspace arithmetic, train.unfreeze_decoder, the arithmetic-mode refusal, and the
float64 restatement of the learning check that tests/test_gpu_decoder_finetune.py repeats on the HIP path."""
import ctypes

import pytest
import torch

import decoder_finetune_cases as fc

EINVAL = -1


def _lib():
    from multimodal_vqvae_compression_audio_tactile_amd import _lib
    return _lib.lib()


def test_exports_are_bound_and_abi_stays_3():
    lib = _lib()
    assert lib.mvq_abi_version() == 3
    for name in ("mvq_conv1d_wgrad_workspace_bytes", "mvq_conv1d_wgrad_f32", "mvq_channel_reduce_workspace_bytes", "mvq_snake_bwd_f32",
                 "mvq_bias_grad_f32", "mvq_weight_norm_bwd_f32"):
        assert hasattr(lib, name), name


def test_workspace_query_follows_the_documented_split():
    """nsplit = min(chunks, ceil(1024 / block tiles), 4096); bytes = nsplit * M * N * ks * 4, 0 when nsplit = 1 or the geometry is
    refused.  A function of the shape alone."""
    q = _lib().mvq_conv1d_wgrad_workspace_bytes
    # 96 x 96 x 7 at 6 x 24 000 tokens: 2 x 2 tiles of 64 -> 256 splits of the 6 * 375 chunks of 64 tokens
    assert q(6, 96, 24000, 96, 24000, 7, 1, 9, 27, 0) == 256 * 96 * 96 * 7 * 4
    # one chunk: nothing to split
    assert q(1, 96, 5, 96, 5, 7, 1, 1, 3, 0) == 0
    # ragged: 2 x ceil(6001 / 64) = 188 chunks, 1 tile -> 188 splits of one chunk each
    assert q(2, 32, 6001, 32, 6001, 7, 1, 1, 3, 0) == 188 * 32 * 32 * 7 * 4
    # the final conv (cout = 1): reduction form, 672 (n, k) blocks -> 2 splits of the 6 * 24 chunks of 1024 tokens
    assert q(6, 96, 24000, 1, 24000, 7, 1, 1, 3, 0) == 2 * 96 * 7 * 4
    # transposed, stride 8: 16-token chunks, two groups of 8 taps
    assert q(2, 192, 75, 96, 600, 16, 8, 1, 4, 1) == min(2 * 5, -(-1024 // (3 * 2 * 2))) * 192 * 96 * 16 * 4
    # refused geometries answer 0
    assert q(2, 32, 75, 32, 74, 7, 1, 1, 3, 0) == 0
    assert q(2, 64, 75, 32, 150, 5, 2, 1, 1, 1) == 0


@pytest.mark.parametrize("geo,why", [
    ((2, 32, 75, 32, 74, 7, 1, 1, 3, 0), "tout"),                     # tout != tin + 2 pad - dil (ks - 1)
    ((2, 64, 75, 32, 150, 5, 2, 1, 1, 1), "2*stride"),                # transposed: ks != 2 * stride
    ((2, 32, 75, 32, 75, 7, 2, 1, 3, 0), "stride 1"),                 # Conv1d form with a stride
    ((2, 64, 75, 32, 200, 4, 2, 1, 1, 1), "tout"),                    # transposed: output_padding >= stride
])
def test_wgrad_refuses_bad_geometry_before_touching_anything(geo, why):
    """The geometry is judged first: with every pointer NULL the call still answers MVQ_EINVAL and names the reason."""
    lib = _lib()
    rc = lib.mvq_conv1d_wgrad_f32(None, None, None, None, None, 0, *geo, None)
    assert rc == EINVAL
    assert why in lib.mvq_last_error().decode()


def test_wgrad_refuses_a_short_workspace_and_null_tensors():
    lib = _lib()
    geo = (2, 32, 6001, 32, 6001, 7, 1, 1, 3, 0)
    need = lib.mvq_conv1d_wgrad_workspace_bytes(*geo)
    assert need > 0
    buf = (ctypes.c_float * 8)()                                       # stands in for every pointer: the refusal comes before any use
    p = ctypes.addressof(buf)
    assert lib.mvq_conv1d_wgrad_f32(p, p, None, p, p, need - 1, *geo, None) == EINVAL
    assert "workspace" in lib.mvq_last_error().decode()
    assert lib.mvq_conv1d_wgrad_f32(p, p, None, p, None, need, *geo, None) == EINVAL
    assert lib.mvq_conv1d_wgrad_f32(None, p, None, p, p, need, *geo, None) == EINVAL
    assert lib.mvq_conv1d_wgrad_f32(p, p, None, None, p, need, *geo, None) == EINVAL


def test_channel_reduce_refusals():
    lib = _lib()
    assert lib.mvq_channel_reduce_workspace_bytes(6, 96, 24000) == 96 * 21 * 4          # min(6 * 12 slabs, 2048 / 96 = 21 ranges)
    assert lib.mvq_channel_reduce_workspace_bytes(1, 1536, 75) == 1536 * 4
    assert lib.mvq_channel_reduce_workspace_bytes(0, 96, 75) == 0
    buf = (ctypes.c_float * 8)()
    p = ctypes.addressof(buf)
    need = lib.mvq_channel_reduce_workspace_bytes(6, 96, 24000)
    assert lib.mvq_snake_bwd_f32(p, p, p, None, p, p, p, need - 1, 6, 96, 24000, None) == EINVAL
    assert "workspace" in lib.mvq_last_error().decode()
    assert lib.mvq_snake_bwd_f32(p, p, None, None, p, None, None, 0, 6, 96, 24000, None) == EINVAL       # no alpha
    assert lib.mvq_bias_grad_f32(p, p, p, need - 1, 6, 96, 24000, None) == EINVAL
    assert lib.mvq_bias_grad_f32(p, None, p, need, 6, 96, 24000, None) == EINVAL
    assert lib.mvq_weight_norm_bwd_f32(p, p, p, p, p, 4, 0, None) == EINVAL
    assert lib.mvq_weight_norm_bwd_f32(p, p, p, None, None, 4, 7, None) == EINVAL


def test_ops_have_no_cpu_fallback():
    from multimodal_vqvae_compression_audio_tactile_amd import ops
    from multimodal_vqvae_compression_audio_tactile_amd._lib import MvqError
    x = torch.zeros(1, 4, 8)
    for call in (lambda: ops.conv1d_wgrad(x, x, 7, pad=3), lambda: ops.snake_bwd(x, x, torch.ones(4)), lambda: ops.bias_grad(x),
                 lambda: ops.weight_norm_bwd(x, x, torch.ones(1, 1, 1))):
        with pytest.raises(MvqError):
            call()


def test_unfreeze_decoder_selects_and_returns_the_parameters():
    from multimodal_vqvae_compression_audio_tactile_amd import Decoder, train
    dec = Decoder(**fc.SMALL)
    for p in dec.parameters():
        p.requires_grad_(False)

    class Net:
        T_DEC = dec

    ps = train.unfreeze_decoder(Net())
    assert len(ps) == len(list(dec.parameters())) and all(p.requires_grad for p in dec.parameters())
    assert [n for n, _ in dec.trainable()] == [n for n, _ in dec.named_parameters()]
    ps = train.unfreeze_decoder(dec, snake=False, bias=False)           # the decoder itself is accepted too
    kinds = {n.rsplit(".", 1)[-1]: p.requires_grad for n, p in dec.named_parameters()}
    assert kinds == {"weight_g": True, "weight_v": True, "bias": False, "alpha": False}
    assert len(ps) == sum(p.requires_grad for p in dec.parameters()) and all(p.requires_grad for p in ps)
    ps = train.unfreeze_decoder(dec, snake=True, bias=False)
    assert {n.rsplit(".", 1)[-1] for n, _ in dec.trainable()} == {"weight_g", "weight_v", "alpha"}


def test_model_constructors_still_freeze_the_decoder():
    from multimodal_vqvae_compression_audio_tactile_amd import AllPredAR, build_proposed
    net = build_proposed(None, rvq_books=3, rvq_embed=128, device="cpu", cls=AllPredAR)
    assert not any(p.requires_grad for p in net.T_DEC.parameters())


def test_trainable_decoder_is_refused_in_the_opt_in_arithmetic_modes():
    """One clear MvqError, before anything runs (so it shows without a device)."""
    from multimodal_vqvae_compression_audio_tactile_amd import Decoder, ops
    from multimodal_vqvae_compression_audio_tactile_amd._lib import MvqError
    dec = Decoder(**fc.SMALL)
    assert not any(p.requires_grad for p in dec.parameters())       # built frozen: training it is opt-in
    dec.model[0].bias.requires_grad_(True)
    z = torch.zeros(1, fc.SMALL["input_channel"], 4)
    for mode in ("bf16x6", "f16x3"):
        with ops.arith(mode), torch.enable_grad():
            with pytest.raises(MvqError, match="trainable decoder runs in the 'f32' arithmetic only"):
                dec(z)
    assert ops.get_arith() == "f32"


def test_backward_params_refuses_the_stack_blob():
    from multimodal_vqvae_compression_audio_tactile_amd import Decoder
    from multimodal_vqvae_compression_audio_tactile_amd._lib import MvqError
    dec = Decoder(**fc.SMALL)
    with pytest.raises(MvqError, match="dict form"):
        dec.backward_params({"blob": object(), "batch": 1, "z_len": 4}, torch.zeros(1, 1, 8))


def test_learning_check_decreases_in_the_float64_restatement():
    """The lr / seed of the GPU learning test, on the yardstick: five AdamW steps on the fixed batch, final L1 strictly below the
    first (and the fp32 restatement agrees)."""
    l64 = fc.learn_oracle(torch.float64)
    l32 = fc.learn_oracle(torch.float32)
    print("float64 losses", l64, "float32 losses", l32)
    assert l64[-1] < l64[0] and l32[-1] < l32[0]
    assert l64[0] - l64[-1] > 1e-3 * l64[0]               # a margin fp32 round-off cannot eat
