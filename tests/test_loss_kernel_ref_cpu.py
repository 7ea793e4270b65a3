"""The per-kernel float64 restatements (tests/loss_kernel_ref.py) compose to the loss oracle: chained frames -> DFT ->
magnitude -> terms -> spec_grad -> transposed DFT -> overlap-add, they reproduce value and autograd d loss / d y of
oracle/losses_torch.py evaluated in float64.  Bars: 1e-9 relative L2 for mrstft and safe_l1 (measured <= 2e-15), 1e-6 for
melcos (measured <= 3e-8; its argmax path is part of the chain) -- far above float64 noise, far below any fp32 effect.
This is what lets tests/test_gpu_loss_kernels.py trust each restatement on its own.  No GPU."""
import pytest
import torch

import loss_kernel_ref as R
from oracle import losses_torch as LT


def _pair(B, T, seed):
    g = torch.Generator().manual_seed(seed)
    tgt = 0.3 * torch.randn(B, T, generator=g, dtype=torch.float64)
    y = tgt + 0.05 * torch.randn(B, T, generator=g, dtype=torch.float64)
    return y, tgt


def _rel(got, want):
    return float((got - want).norm() / want.norm().clamp_min(1e-300))


@torch.enable_grad()
def _oracle(fn, y, tgt):
    yr = y.clone().unsqueeze(1).requires_grad_(True)
    v = fn(yr, tgt.unsqueeze(1))
    v.backward()
    return float(v.detach()), yr.grad[:, 0]


def _check(name, got, want, bar):
    (v, dy), (vo, dyo) = got, want
    err = _rel(dy, dyo)
    print(f"{name}: value {float(v):.15g} vs {vo:.15g}, dL/dy relative L2 {err:.2e}")
    assert abs(float(v) - vo) <= bar * abs(vo)
    assert err <= bar


@pytest.mark.parametrize("B,T", [(1, 129), (3, 191), (2, 513), (2, 1000), (3, 5600)])
def test_mrstft_chain_matches_oracle(B, T):
    y, tgt = _pair(B, T, 100 + T)
    _check("mrstft", R.mrstft_chain(y, tgt), _oracle(LT.mrstft, y, tgt), 1e-9)


@pytest.mark.parametrize("B,T", [(1, 257), (3, 700), (2, 2000)])
def test_melcos_chain_matches_oracle(B, T):
    y, tgt = _pair(B, T, 200 + T)
    _check("melcos", R.melcos_chain(y, tgt, LT.mel_filterbank()), _oracle(LT.melcos, y, tgt), 1e-6)


@pytest.mark.parametrize("B,T", [(1, 1), (3, 191), (2, 1000)])
def test_l1_chain_matches_oracle(B, T):
    y, tgt = _pair(B, T, 300 + T)
    if T > 4:
        y[0, 3] = tgt[0, 3]                                              # sign(0) = 0
    _check("safe_l1", R.l1_chain(y, tgt), _oracle(LT.safe_l1, y, tgt), 1e-9)


def test_short_clip_falls_back_to_l1():
    y, tgt = _pair(2, 100, 7)
    _check("mrstft T=100", R.mrstft_chain(y, tgt), _oracle(LT.mrstft, y, tgt), 1e-9)


@pytest.mark.parametrize("name", ["safe_l1", "mrstft"])
def test_non_finite_prediction_samples(name):
    """The kernels' contracts sanitise values; the oracle's nan_to_num also gives those samples gradient 0.  The chain
    times isfinite(y) -- the rule losses._evaluate applies -- is the oracle's gradient."""
    y, tgt = _pair(2, 700, 9)
    for b, t, v in ((0, 0, float("nan")), (0, 17, float("inf")), (1, 699, float("-inf")), (1, 17, float("nan"))):
        y[b, t] = v
    tgt[1, 99] = float("inf")
    chain, fn = (R.l1_chain, LT.safe_l1) if name == "safe_l1" else (R.mrstft_chain, LT.mrstft)
    v, dy = chain(y, tgt)
    vo, dyo = _oracle(fn, y, tgt)
    assert bool((dyo[~torch.isfinite(y)] == 0).all())
    assert bool((dy[~torch.isfinite(y)] != 0).any())
    _check(name, (v, dy * torch.isfinite(y)), (vo, dyo), 1e-9)
