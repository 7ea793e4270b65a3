"""Float64 restatements of the optimiser and element-wise training kernels' contracts (csrc/kernels_bwd.hip: gelu_bwd,
scale_tanh, scale_tanh_bwd, mul_scaled, transpose2d, rowsum, sumsq_partial, adamw; csrc/kernels_small.hip: mul_dtanh,
strided3d, gelu), one function per kernel -- test infrastructure, no test in here.  Each is written from the kernel's header
comment and the reference's formula (nn.GELU, scale * tanh(TokenNorm(r)), torch.optim.AdamW / clip_grad_norm_ of
Training/compare_dacvsproposal_5.py:229-241,313-315,367,394), in plain torch on the CPU.

tests/test_train_kernel_ref_cpu.py holds them against torch autograd and torch.optim.AdamW in float64, so that a
misconception shared by a kernel and its restatement cannot hide.

The elementary functions of csrc/det_math.hpp are not restated here (oracle/c/det_math.h reproduces their bits); what this file
holds of them is the error ALLOWANCE a bounded comparison against the true function may grant them, derived from their
definitions (``tanh_allowance``, ``EXP_REL``, ``ERF_AS``) and never from what a kernel returns.
"""
import math

import numpy as np
import torch

U = 2.0 ** -24                     # unit roundoff of fp32
F64 = torch.float64
BLOCK = 256                        # threads per block of every kernel here


def f32(v):
    """The value a C float argument takes, as a Python float."""
    return float(np.float32(v))


# ---- GELU ------------------------------------------------------------------------------------------------------------------
def gelu(x):
    x = x.to(F64)
    return 0.5 * x * (1.0 + torch.special.erf(x / math.sqrt(2.0)))


def gelu_grad(x):
    """GELU'(x) = Phi(x) + x * phi(x)."""
    x = x.to(F64)
    cdf = 0.5 * torch.special.erfc(-x / math.sqrt(2.0))                  # erfc: no cancellation in the left tail
    pdf = torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    return cdf + x * pdf


def gelu_bwd(x, g):
    return g.to(F64) * gelu_grad(x)


# ---- s * tanh(u) -----------------------------------------------------------------------------------------------------------
def scale_tanh(u, s):
    return s * torch.tanh(u.to(F64))


def block_of(n, n_partial):
    """Element i of a flat tensor is summed by block (i / 256) % n_partial: the grid-stride loop of a grid of n_partial
    blocks of 256 threads."""
    return (torch.arange(n, dtype=torch.int64) // BLOCK) % n_partial


def block_sums(values, n_partial):
    """Per-block float64 sums of a flat tensor under ``block_of``; a block without elements sums to 0."""
    values = values.to(F64).reshape(-1)
    out = torch.zeros(n_partial, dtype=F64)
    if values.numel():
        out.index_add_(0, block_of(values.numel(), n_partial), values)
    return out


def serial_terms(n, n_partial):
    """Most terms one thread adds up: ceil(n / (256 * n_partial))."""
    return -(-n // (BLOCK * n_partial))


def scale_tanh_bwd(u, g, s, n_partial):
    """-> (gu = g*s*(1 - tanh^2 u), partial[n_partial] = per-block sums of g*tanh u, dscale = sum g*tanh u)."""
    u, g = u.to(F64).reshape(-1), g.to(F64).reshape(-1)
    t = torch.tanh(u)
    # 1 - tanh^2 = sech^2 without the cancellation at large |u|
    sech2 = 1.0 / torch.cosh(u) ** 2
    return g * s * sech2, block_sums(g * t, n_partial), (g * t).sum()


def mul_dtanh(g, y):
    """g * (1 - y^2), y being a saved tanh output."""
    return g.to(F64) * (1.0 - y.to(F64) ** 2)


# ---- plain data movement and sums -------------------------------------------------------------------------------------------
def mul_scaled(a, b, scale):
    return a.to(F64) * b.to(F64) * scale


def transpose2d(x):
    return x.t().contiguous()


def rowsum(x, out0=None):
    """x [rows, cols] -> [rows]; with out0 the kernel's accumulate form out0 + sum."""
    s = x.to(F64).sum(1)
    return s if out0 is None else out0.to(F64) + s


def sumsq_partials(x, n_partial):
    x = x.to(F64).reshape(-1)
    return block_sums(x * x, n_partial)


def grad_norm(tensors):
    return math.sqrt(sum(float((t.to(F64) ** 2).sum()) for t in tensors))


def clip_coef(total_norm, max_norm):
    """torch.nn.utils.clip_grad_norm_'s factor."""
    return min(1.0, max_norm / (total_norm + 1e-6))


def copy3d(dst, dst_off, dst_strides, src, src_off, src_strides, B, C, n, minus=None):
    """The strided3d contract on flat tensors: dst[dst_off + b*ds0 + c*ds1 + t] = src[src_off + b*ss0 + c*ss1 + t]
    (- minus[the same source offsets]) for b < B, c < C, t < n.  Returns a new flat tensor; dst is not changed."""
    out = dst.reshape(-1).clone()
    if B * C * n == 0:
        return out
    b = torch.arange(B).reshape(B, 1, 1); c = torch.arange(C).reshape(1, C, 1); t = torch.arange(n).reshape(1, 1, n)
    si = (src_off + b * src_strides[0] + c * src_strides[1] + t).reshape(-1)
    di = (dst_off + b * dst_strides[0] + c * dst_strides[1] + t).reshape(-1)
    v = src.reshape(-1)[si]
    if minus is not None:
        v = v - minus.reshape(-1)[si]
    out[di] = v
    return out


# ---- AdamW -----------------------------------------------------------------------------------------------------------------
def adamw_abi_hyper(lr, beta1, beta2, eps, weight_decay, step):
    """The hyper-parameters as the kernel receives them: every one rounded to fp32 by the C ABI, the bias corrections computed
    in double FROM the fp32 betas and then rounded to fp32 (mvq_adamw_f32 in csrc/api.hip)."""
    b1, b2 = f32(beta1), f32(beta2)
    return dict(lr=f32(lr), beta1=b1, beta2=b2, eps=f32(eps), weight_decay=f32(weight_decay),
                bc1=f32(1.0 - b1 ** step), sqrt_bc2=f32(math.sqrt(1.0 - b2 ** step)))


def adamw_exact_hyper(lr, beta1, beta2, eps, weight_decay, step):
    """The same in unrounded double: what torch.optim.AdamW computes with on double parameters."""
    return dict(lr=lr, beta1=beta1, beta2=beta2, eps=eps, weight_decay=weight_decay,
                bc1=1.0 - beta1 ** step, sqrt_bc2=math.sqrt(1.0 - beta2 ** step))


def adamw_step(p, g, m, v, h, coef=1.0):
    """One step in torch's single-tensor order (the comment above adamw_kernel):
        g *= coef;  p *= 1 - lr*wd;  m = b1*m + (1-b1)*g;  v = b2*v + (1-b2)*g*g;  p -= (lr/bc1) * m / (sqrt(v)/sqrt(bc2) + eps)
    in float64 with the hyper-parameters ``h`` taken as they are.  -> (p, m, v), new tensors."""
    p, g, m, v = (t.to(F64) for t in (p, g, m, v))
    g = g * coef
    p = p * (1.0 - h["lr"] * h["weight_decay"])
    m = h["beta1"] * m + (1.0 - h["beta1"]) * g
    v = h["beta2"] * v + (1.0 - h["beta2"]) * g * g
    denom = v.sqrt() / h["sqrt_bc2"] + h["eps"]
    p = p - (h["lr"] / h["bc1"]) * (m / denom)
    return p, m, v


# ---- what the device's elementary functions may be off by, from their definitions in csrc/det_math.hpp ------------------------
# det_exp(x) = (1 + P(r)) * 2^n, r = x - n*ln2 by a two-constant Cody-Waite reduction (both fma: the first is exact, the second
# rounds once, |dr| <= u*|r| <= 0.35u; the split constant is ln2 to 2e-4 u over |n| <= 127), P the degree-7 Taylor polynomial of
# exp(r) - 1 on |r| <= ln2/2 (truncation r^8/8! <= 5.2e-9 = 0.09u; Horner roundings of p <= 0.57 carried through r*r*p <= 0.07:
# 0.17u; the closing fma u*|P| <= 0.42u), then one rounding of 1 + P and an exact power of two.  Relative to e^r in
# [0.707, 1.414] the sum is 2.1u at the lower end and 1.9u at the upper:
EXP_REL = 2.5                      # |det_exp(x) - e^x| <= EXP_REL * u * e^x for -87 <= x <= 88
# det_erf is Abramowitz & Stegun 7.1.26: |eps| <= 1.5e-7 in exact arithmetic
ERF_AS = 1.5e-7 / U                # = 2.52 u, absolute


def tanh_allowance(x):
    """|det_tanh(x) - tanh(x)| <= this (absolute, float64 tensor), branch by branch:
      |x| < 0.17:  em1 = P(2|x|) with relative error <= 1.6u (closing fma u, the r*r*p part and the truncation 0.6u of em1),
                   em1 / (em1 + 2): em1's error enters with weight 2/(em1+2) <= 1, the add and the division round once
                   each: <= 3.6u relative;
      |x| > 10:    returns 1: off by 1 - tanh|x| = 2 e^-2|x| / (1 + e^-2|x|) <= 4.2e-9 = 0.07u;
      otherwise:   t = det_exp(-2|x|) (EXP_REL*u relative), (1 - t) / (1 + t): d/dt = -2/(1+t)^2, three roundings:
                   <= u * (2*EXP_REL*t/(1+t)^2 + 3*tanh|x|)."""
    a = x.to(F64).abs()
    th = torch.tanh(a)
    t = torch.exp(-2.0 * a)
    mid = U * (2.0 * EXP_REL * t / (1.0 + t) ** 2 + 3.0 * th)
    small = 3.6 * U * th
    big = 2.0 * t / (1.0 + t)
    return torch.where(a < f32(0.17), small, torch.where(a > 10.0, big, mid))


_AS = (0.254829592, -0.284496736, 1.421413741, -1.453152027, 1.061405429)      # a1 .. a5 of A&S 7.1.26, p = 0.3275911


def gelu_grad_allowance(x):
    """|device GELU'(x) - GELU'(x)| <= this (absolute, float64 tensor) for gelu_bwd_kernel's chain
        z = x * fl(1/sqrt 2);  t = 1 / fma(p, |z|, 1);  P = Horner(a5..a1; t) * t;  erf = 1 - P * det_exp(-z*z);
        cdf = 0.5 * (1 + erf);  pdf = fl(1/sqrt(2 pi)) * det_exp(-0.5*x*x);  d = fma(x, pdf, cdf)
    by first-order propagation of every rounding, the A&S formula's own error and det_exp's allowance:
      z:    one product and the constant's rounding (0.29u): |dz| <= 1.3u|z|, worth erf'(z)*|dz| on erf;
      t:    the fma and the division, plus p's rounding (weight 1 - t): relative (2 + 0.5(1 - t))u, worth |t P'(t)| of that;
      P:    five Horner roundings u*|p_k| carried through the remaining powers of t, and the five fp32 coefficients' own
            (known) roundings;
      e:    z*z rounds once (relative u*z^2 on e) and det_exp is off by EXP_REL*u;
      erf:  e*dP + P*e*(z^2 + EXP_REL)u + u|erf| (the closing fma) + ERF_AS*u;
      cdf:  half of that, and u*cdf for 1 + erf;
      pdf:  -0.5*x*x rounds once (relative u*x^2/2), det_exp, the product with the constant and the constant: (x^2/2 + EXP_REL + 1.5)u;
      d:    dcdf + |x|*dpdf + u|d|.
    The product with g rounds once more: gelu_bwd's bound is |g| * (this + u*|GELU'|)."""
    x = x.to(F64)
    z = x / math.sqrt(2.0)
    a = z.abs()
    t = 1.0 / (1.0 + 0.3275911 * a)
    a1, a2, a3, a4, a5 = _AS
    p1 = a5 * t + a4; p2 = t * p1 + a3; p3 = t * p2 + a2; p4 = t * p3 + a1; P = p4 * t
    horner = U * (p1.abs() * t ** 4 + p2.abs() * t ** 3 + p3.abs() * t ** 2 + p4.abs() * t + P.abs())
    coef = sum((float(np.float32(c)) - c) * t ** (k + 1) for k, c in enumerate(_AS)).abs()
    dP_t = sum((k + 1) * c * t ** (k + 1) for k, c in enumerate(_AS)).abs() * (2.0 + 0.5 * (1.0 - t)) * U
    e = torch.exp(-a * a)
    erf = torch.special.erf(a)
    d_erf = (e * (horner + coef + dP_t) + P * e * (a * a + EXP_REL) * U + U * erf + ERF_AS * U
             + 2.0 / math.sqrt(math.pi) * e * 1.3 * U * a)
    cdf = 0.5 * torch.special.erfc(-z)
    pdf = torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    d = cdf + x * pdf
    return 0.5 * d_erf + U * cdf + x.abs() * pdf * (0.5 * x * x + EXP_REL + 1.5) * U + U * d.abs()
