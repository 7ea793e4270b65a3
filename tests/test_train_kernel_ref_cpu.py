"""The per-kernel float64 restatements of tests/train_kernel_ref.py against independent float64 truth: torch autograd for
GELU' and the scale-tanh gradients, torch.optim.AdamW (+ clip_grad_norm_) on double parameters for the AdamW order, naive
loops for the block mapping and the strided copy.  This is what lets tests/test_gpu_train_kernels.py trust each restatement on
its own.  Measured: GELU' 2.3e-16 absolute, scale-tanh 3e-16 relative, AdamW over 5 steps <= 5e-16 relative (bar 1e-12).

Also here, because it needs no GPU: what rounding the hyper-parameters to fp32 (the C ABI takes floats) does to a step, and
that optim.AdamW refuses a parameter that is not fp32 before anything is launched.  No GPU."""
import math

import pytest
import torch

import train_kernel_ref as R

F64 = torch.float64
U = R.U


def _gen(seed):
    return torch.Generator().manual_seed(seed)


@torch.enable_grad()
def test_gelu_grad_matches_autograd():
    x = torch.cat([torch.linspace(-12, 12, 4801, dtype=F64), torch.tensor([-0.7518, 0.0, 1e-9, -40.0, 40.0], dtype=F64)])
    g = torch.randn(x.numel(), generator=_gen(1), dtype=F64)
    xr = x.clone().requires_grad_(True)
    torch.nn.functional.gelu(xr).backward(g)
    err = float((R.gelu_bwd(x, g) - xr.grad).abs().max())
    print(f"gelu_bwd: largest absolute difference from autograd {err:.2e}")
    assert err <= 1e-14
    assert float((R.gelu(x) - torch.nn.functional.gelu(x)).abs().max()) <= 1e-14
    # the zero of GELU' that the GPU test plants: between -0.7518 and -0.7517
    assert float(R.gelu_grad(torch.tensor([-0.7518]))) < 0 < float(R.gelu_grad(torch.tensor([-0.7517])))


@torch.enable_grad()
@pytest.mark.parametrize("n,n_partial", [(1, 1), (257, 2), (1000, 3), (5000, 4)])
def test_scale_tanh_grads_match_autograd(n, n_partial):
    g_ = _gen(2 + n)
    u = 4.0 * torch.randn(n, generator=g_, dtype=F64)
    if n > 1:
        u[0] = 12.0                                                      # 1 - tanh^2 cancels in autograd here: seen against the largest gradient only
    g = torch.randn(n, generator=g_, dtype=F64)
    s = 0.37
    ur = u.clone().requires_grad_(True); sr = torch.tensor(s, dtype=F64, requires_grad=True)
    y = sr * torch.tanh(ur)
    y.backward(g)
    gu, partial, dscale = R.scale_tanh_bwd(u, g, s, n_partial)
    assert float((R.scale_tanh(u, s) - y.detach()).abs().max()) == 0.0
    err = float((gu - ur.grad).abs().max() / ur.grad.abs().max())
    print(f"scale_tanh_bwd[{n}]: gu {err:.2e}, dscale {abs(float(dscale) - float(sr.grad)):.2e}")
    assert err <= 1e-14
    assert abs(float(dscale) - float(sr.grad)) <= 1e-13 * float((g * torch.tanh(u)).abs().sum())
    assert abs(float(partial.sum()) - float(dscale)) <= 1e-13 * float((g * torch.tanh(u)).abs().sum())
    assert float((R.mul_dtanh(g, torch.tanh(u)) * s - ur.grad).abs().max()) <= 1e-14 * float(ur.grad.abs().max())


@pytest.mark.parametrize("n,n_partial", [(0, 4), (1, 4), (256, 1), (257, 2), (256 * 3 + 5, 3), (256 * 7 + 1, 3)])
def test_block_mapping_is_the_grid_stride_loop(n, n_partial):
    """block_sums against the loop as the kernels write it: block b, thread t walks i = b*256 + t, += n_partial*256."""
    vals = torch.randn(n, generator=_gen(3 + n), dtype=F64)
    want = torch.zeros(n_partial, dtype=F64)
    longest = 0
    for b in range(n_partial):
        for t in range(256):
            idx = range(b * 256 + t, n, n_partial * 256)
            longest = max(longest, len(idx))
            for i in idx:
                want[b] += vals[i]
    assert float((R.block_sums(vals, n_partial) - want).abs().max()) <= 1e-13
    assert R.serial_terms(n, n_partial) >= longest and (n == 0 or R.serial_terms(n, n_partial) == longest)
    assert float((R.sumsq_partials(vals, n_partial).sum() - (vals * vals).sum()).abs()) <= 1e-12


def test_copy3d_is_torch_indexing():
    B, C, T, s, n = 3, 5, 11, 4, 6
    a = torch.randn(B, C, T, generator=_gen(4))
    # fold_time_slice: [B,C,T][..., s:s+n] -> [C, B*n]
    got = R.copy3d(torch.zeros(C * B * n), 0, (n, B * n), a, s, (C * T, T), B, C, n).reshape(C, B * n)
    assert torch.equal(got, a[:, :, s:s + n].permute(1, 0, 2).reshape(C, B * n))
    # a zero stride repeats the source; minus subtracts at the source offsets
    row = torch.randn(n, generator=_gen(5))
    got = R.copy3d(torch.zeros(B * C * n), 0, (C * n, n), row, 0, (0, 0), B, C, n).reshape(B, C, n)
    assert torch.equal(got, row.expand(B, C, n))
    b = torch.randn(B, C, T, generator=_gen(6))
    got = R.copy3d(torch.zeros(B * C * T), 0, (C * T, T), a, 0, (C * T, T), B, C, T, minus=b).reshape(B, C, T)
    assert torch.equal(got, a - b)
    assert torch.equal(R.transpose2d(a[0]), a[0].T) and R.transpose2d(a[0]).is_contiguous()
    assert float((R.rowsum(a[0], a[0, :, 0]) - (a[0].double().sum(1) + a[0, :, 0].double())).abs().max()) == 0.0


# ---- AdamW -----------------------------------------------------------------------------------------------------------------
HYPER = [dict(lr=2e-4, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-5),
         dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.1)]
SHAPES = [(7, 5), (33,), ()]


def _grads(step, big):
    g_ = _gen(100 + step)
    scale = 40.0 if big else 0.02                                         # 40: norm far above the clip threshold of 3
    return [scale * torch.randn(s, generator=g_, dtype=F64) for s in SHAPES]


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("hyper", HYPER)
def test_adamw_restatement_matches_torch_double(hyper, clip):
    """5 steps of torch.optim.AdamW on double parameters, with and without clip_grad_norm_(3.0); the restatement with the
    unrounded hyper-parameters follows it to 1e-12 relative (measured <= 5e-16)."""
    params = [torch.randn(s, generator=_gen(7), dtype=F64).requires_grad_(True) for s in SHAPES]
    opt = torch.optim.AdamW(params, lr=hyper["lr"], betas=(hyper["beta1"], hyper["beta2"]), eps=hyper["eps"],
                            weight_decay=hyper["weight_decay"])
    mine = [(p.detach().clone(), torch.zeros_like(p), torch.zeros_like(p)) for p in params]
    worst = 0.0
    for step in range(1, 6):
        grads = _grads(step, big=step % 2 == 0)
        for p, g in zip(params, grads):
            p.grad = g.clone()
        coef = 1.0
        if clip:
            coef = R.clip_coef(R.grad_norm(grads), 3.0)
            total = torch.nn.utils.clip_grad_norm_(params, 3.0)
            assert abs(float(total) - R.grad_norm(grads)) <= 1e-12 * float(total)
            assert (coef < 1.0) == (step % 2 == 0)
        opt.step()
        h = R.adamw_exact_hyper(step=step, **hyper)
        mine = [R.adamw_step(p, g, m, v, h, coef) for (p, m, v), g in zip(mine, grads)]
        for (p, m, v), tp in zip(mine, params):
            st = opt.state[tp]
            for got, want in ((p, tp.detach()), (m, st["exp_avg"]), (v, st["exp_avg_sq"])):
                worst = max(worst, float((got - want).abs().max() / want.abs().max()))
    print(f"adamw restatement vs torch double, 5 steps, clip={clip}, wd={hyper['weight_decay']}: {worst:.2e}")
    assert worst <= 1e-12


@pytest.mark.parametrize("hyper", HYPER)
def test_fp32_hyper_parameters_move_a_step_by_a_few_u(hyper):
    """The C ABI takes lr, betas, eps and weight_decay as floats and rounds the bias corrections to fp32.  Each rounding is a
    relative change of at most u = 2^-24 (round to nearest).  For the state of a run from zero at step t,
        m / bc1 = sum_i w_i g_i,  w_i = (1-b1) b1^(t-i) / (1 - b1^t),  sum_i w_i = 1,
    and d ln w_i / d ln b1 = (t - i) - b1/(1-b1) + t b1^t/(1-b1^t): linear in i with range t - 1 and w-weighted mean 0, so
    |d ln w_i / d ln b1| <= t - 1 -- the large factors b/(1-b) (9 and 999) cancel against the bias correction, which api.hip
    computes from the SAME fp32 beta.  So rounding b1 moves m/bc1 by at most (t-1) u sum_i w_i |g_i|, rounding b2 moves v/bc2 by at
    most (t-1) u v/bc2 (its terms are non-negative), i.e. its square root by (t-1)/2 u.  Rounding bc1 and sqrt(bc2) themselves:
    u each; eps: at most u of the denominator's eps share; lr: u on both parts of the update; weight_decay: u on the decay.
    Summed, with D = sqrt(v/bc2) + eps and A = lr * (m/bc1) / D the Adam part of the update:
        |d update| <= u * ( 2 lr wd |p|  +  |A| * (1 [lr] + 1 [bc1] + 1 [sqrt bc2 | eps] + (t-1)/2 [b2])
                            + (lr / D) * (t-1) * sum_i w_i |g_i| [b1] )
    which for t <= 5 is 'a few u' of the terms the update is made of.  A margin of 1.05 covers second order."""
    n = 4000
    p = torch.randn(n, generator=_gen(8), dtype=F64)
    mag = torch.exp(math.log(1e-9) + (math.log(1e2) - math.log(1e-9)) * torch.rand(n, generator=_gen(9), dtype=F64))
    worst = 0.0
    states = {"abi": (torch.zeros(n, dtype=F64), torch.zeros(n, dtype=F64)), "exact": (torch.zeros(n, dtype=F64), torch.zeros(n, dtype=F64))}
    wabs = torch.zeros(n, dtype=F64)                                     # sum_i w_i |g_i|, carried as an unnormalised recurrence
    for t in range(1, 6):
        g = mag * torch.randn(n, generator=_gen(10 + t), dtype=F64)
        out = {}
        for name, make in (("abi", R.adamw_abi_hyper), ("exact", R.adamw_exact_hyper)):
            h = make(step=t, **hyper)
            m, v = states[name]
            pn, mn, vn = R.adamw_step(p, g, m, v, h)
            states[name] = (mn, vn)
            out[name] = pn - p
        b1, lr, wd = hyper["beta1"], hyper["lr"], hyper["weight_decay"]
        wabs = b1 * wabs + (1 - b1) * g.abs()
        he = R.adamw_exact_hyper(step=t, **hyper)
        me, ve = states["exact"]
        D = ve.sqrt() / he["sqrt_bc2"] + he["eps"]
        A = (lr / he["bc1"]) * me / D
        bound = U * (2 * lr * wd * p.abs() + A.abs() * (3 + (t - 1) / 2) + (lr / D) * (t - 1) * wabs / he["bc1"])
        ratio = float(((out["abi"] - out["exact"]).abs() / (1.05 * bound)).max())
        in_u = float(((out["abi"] - out["exact"]).abs() / (U * (lr * wd * p.abs() + (lr / D) * wabs / he["bc1"]))).max())
        print(f"step {t}, wd={wd}: fp32 hyper-parameters move the update by {in_u:.2f} u of lr*wd*|p| + lr*sum w|g|/D; {ratio:.3f} of the bound")
        worst = max(worst, ratio)
        assert in_u <= 3 + 1.5 * (t - 1)                                 # 'a few u': the bound's coefficients, |A| <= lr*sum w|g|/D
    assert worst <= 1.0


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float64])
def test_adamw_refuses_other_dtypes_before_any_launch(dtype):
    """The dtype is checked before the device and before the first launch, so the refusal shows without a GPU: MvqError names
    the dtype, and neither the parameter nor the optimiser's state has changed."""
    from multimodal_vqvae_compression_audio_tactile_amd import optim
    from multimodal_vqvae_compression_audio_tactile_amd.ops import MvqError
    p = torch.nn.Parameter(torch.randn(4, 3, generator=_gen(11)).to(dtype))
    before = p.detach().clone()
    p.grad = torch.ones_like(p)
    opt = optim.AdamW([p], lr=1e-2)
    with pytest.raises(MvqError, match=str(dtype).replace(".", r"\.")):
        opt.step()
    assert torch.equal(p.detach(), before) and not opt.state[p]
