"""Host only: the dispatch of the three forward launchers that choose a kernel by token count, width and alignment
(ops.layernorm_kernel_name, ops.rvq_ema_forward_kernel_name, ops.dac_rvq_kernel_name: the launchers' own decision functions,
asked without a device), held against the case tables of tests/forward_forms_cases.py -- so that no shape the library can be
handed runs a kernel that tests/test_gpu_forward_forms.py does not pin -- and the oracle those GPU tests compare with, held
against float64 at the very same inputs."""
import itertools

import numpy as np
import pytest
import torch

import forward_forms_cases as fc
from multimodal_vqvae_compression_audio_tactile_amd import ops

GRID_N = (1, 64, 65, 256, 257, 1023, 1024, 1025, 4095, 4096, 8160, 8161, 19200)
MODEL_N = tuple(per_item * B for per_item in (16, 75) for B in (1, 6, 64, 256))      # one AR chunk / one segment per item

LN_HAVE = {c[4] for c in fc.LN_CASES}
RVQ_HAVE = {c[7] for c in fc.RVQ_CASES}
DAC_HAVE = {fc.dac_form(c[7], c[1]) for c in fc.DAC_CASES}


def _ln(n, C):
    return ops.layernorm_kernel_name(1, C, n)


def _rvq(n, D, K, aligned=True):
    return ops.rvq_ema_forward_kernel_name(1, D, n, K, aligned)


def _dac(n, C, K=1024, prepared=True, aligned=True):
    return ops.dac_rvq_kernel_name(1, C, n, K, prepared, aligned)


# ------------------------------------------------------------------------------------------------------------ the tables
def test_every_case_names_the_form_it_runs():
    for c in fc.LN_CASES:
        assert ops.layernorm_kernel_name(c[0], c[1], c[2]) == c[4], fc.ln_id(c)
    for c in fc.RVQ_CASES:
        assert ops.rvq_ema_forward_kernel_name(c[0], c[1], c[2], c[4]) == c[7], fc.rvq_id(c)
    for c in fc.DAC_CASES:
        assert ops.dac_rvq_kernel_name(c[0], c[1], c[2], c[4], c[5]) == fc.dac_form(c[7], c[1]), fc.dac_id(c)


def test_tables_cover_every_form_option_and_edge():
    assert LN_HAVE == set(fc.LN_FORMS) and RVQ_HAVE == set(fc.RVQ_FORMS)
    assert DAC_HAVE == {fc.dac_form(k, C) for k in fc.DAC_KINDS for C in (256, 512, 1024)}
    for form in fc.LN_FORMS:                                       # each option on at least one case of every form
        opts = {c[3] for c in fc.LN_CASES if c[4] == form}
        assert all(o in opts for o in fc.LN_OPTIONS) and () in opts, (form, opts)
    for form in fc.RVQ_FORMS:                                      # one tie case per form, `use < nb` on one case per form
        mine = [c for c in fc.RVQ_CASES if c[7] == form]
        assert any(c[6] for c in mine), form
        assert any(c[5] is not None and c[5] < c[3] for c in mine) or form == fc.RVQ_MFMA32, form
    assert any(c[7] == fc.RVQ_MFMA16 and c[5] is not None and c[5] < c[3] for c in fc.RVQ_CASES)      # ... the MFMA kernel has its own
    for kind in fc.DAC_KINDS:                                      # nq_item on one case per form
        assert any(c[6] is not None for c in fc.DAC_CASES if c[7] == kind), kind
    assert any(c[3] == 32 for c in fc.DAC_CASES)
    for c in fc.DAC_CASES:
        assert c[6] is None or (len(c[6]) == c[0] and all(1 <= n <= c[3] for n in c[6]) and len(set(c[6])) > 1)


# -------------------------------------------------------------------------------------------------------------- the sweep
def test_no_shape_of_the_grid_runs_a_form_without_a_case():
    for n, C in itertools.product(GRID_N, sorted({c[1] for c in fc.LN_CASES})):
        assert _ln(n, C) in LN_HAVE, (n, C, _ln(n, C))
    Ds, Ks = sorted({c[1] for c in fc.RVQ_CASES}), sorted({c[4] for c in fc.RVQ_CASES})
    for n, D, K, al in itertools.product(GRID_N, Ds, Ks, (True, False)):
        assert _rvq(n, D, K, al) in RVQ_HAVE, (n, D, K, al, _rvq(n, D, K, al))
    Cs, Ks = sorted({c[1] for c in fc.DAC_CASES}), sorted({c[4] for c in fc.DAC_CASES})
    for n, C, K, prep, al in itertools.product(GRID_N, Cs, Ks, (True, False), (True, False)):
        assert _dac(n, C, K, prep, al) in DAC_HAVE, (n, C, K, prep, al, _dac(n, C, K, prep, al))


def test_the_shapes_the_models_launch_run_forms_with_a_case():
    assert MODEL_N == (16, 96, 1024, 4096, 75, 450, 4800, 19200)
    for n in MODEL_N:
        assert _ln(n, 1024) in LN_HAVE
        assert _ln(n, 1024) == (fc.LN_LAT if n <= 1024 else fc.LN_T8)
        for K in (128, 512):
            assert _rvq(n, 96, K) in RVQ_HAVE
            assert _rvq(n, 96, K) == (fc.RVQ_ROWS if n <= 256 else fc.RVQ_T8 if n < 1024 else fc.RVQ_MFMA16 if n < 8161 else fc.RVQ_MFMA32)
        assert _dac(n, 1024) in DAC_HAVE
        assert _dac(n, 1024) == fc.dac_form("lat1" if n <= 256 else "lat2" if n <= 1024 else "tile", 1024)


# --------------------------------------------------------------------------------------------------------- the boundaries
def test_layernorm_decision_boundaries():
    assert (_ln(1024, 1024), _ln(1025, 1024)) == (fc.LN_LAT, fc.LN_T8)             # the latency form's token limit
    assert (_ln(5, 64), _ln(5, 72)) == (fc.LN_LAT, fc.LN_T4)                       # ... and its C % 64 == 0
    assert (_ln(1024, 1216), _ln(1024, 1248)) == (fc.LN_LAT, fc.LN_T8)
    assert (_ln(64, 72), _ln(65, 72)) == (fc.LN_T4, fc.LN_T8)                      # 4- against 8-token tiles
    assert (_ln(64, 1278), _ln(65, 1278)) == (fc.LN_T4, fc.LN_T8)
    assert (_ln(5, 1278), _ln(5, 1279)) == (fc.LN_T4, fc.LN_SCALAR)                # the widest tiled C
    assert (_ln(130, 1278), _ln(130, 1279)) == (fc.LN_T8, fc.LN_SCALAR)
    assert (_ln(19200, 1278), _ln(19200, 1279)) == (fc.LN_T8, fc.LN_SCALAR)
    assert (_ln(5, 1216), _ln(5, 1280)) == (fc.LN_LAT, fc.LN_SCALAR)               # a multiple of 64 that is too wide
    assert _ln(19200, 2050) == fc.LN_SCALAR and _ln(1, 1) == fc.LN_T4
    assert ops.layernorm_kernel_name(4, 1024, 256) == fc.LN_LAT and ops.layernorm_kernel_name(5, 1024, 205) == fc.LN_T8    # n = B * T


def test_rvq_search_decision_boundaries():
    assert (_rvq(256, 96, 512), _rvq(257, 96, 512)) == (fc.RVQ_ROWS, fc.RVQ_T8)    # one block per token up to 256
    assert (_rvq(256, 64, 512), _rvq(257, 64, 512)) == (fc.RVQ_TOKEN, fc.RVQ_T8)
    assert (_rvq(16, 96, 512), _rvq(16, 96, 513)) == (fc.RVQ_ROWS, fc.RVQ_TOKEN)   # rows: K <= 512 ...
    assert (_rvq(16, 96, 512), _rvq(16, 92, 512), _rvq(16, 100, 512)) == (fc.RVQ_ROWS, fc.RVQ_TOKEN, fc.RVQ_TOKEN)       # ... D == 96 ...
    assert (_rvq(16, 96, 512, True), _rvq(16, 96, 512, False)) == (fc.RVQ_ROWS, fc.RVQ_TOKEN)                            # ... aligned books
    assert (_rvq(1023, 96, 512), _rvq(1024, 96, 512)) == (fc.RVQ_T8, fc.RVQ_MFMA16)               # MFMA from 1024 tokens ...
    assert (_rvq(1030, 96, 512), _rvq(1030, 96, 500), _rvq(1030, 96, 544)) == (fc.RVQ_MFMA16, fc.RVQ_T8, fc.RVQ_MFMA16)  # ... K % 32 == 0 ...
    assert (_rvq(8160, 96, 512), _rvq(8161, 96, 512)) == (fc.RVQ_MFMA16, fc.RVQ_MFMA32)           # 256 blocks of 32
    assert (_rvq(4095, 32, 100), _rvq(4096, 32, 100)) == (fc.RVQ_T8, fc.RVQ_T32)                  # not eligible: 8- against 32-token tiles
    assert (_rvq(4095, 96, 500), _rvq(4096, 96, 500)) == (fc.RVQ_T8, fc.RVQ_T32)
    # ... fits LDS: D = 124 is the widest for the MFMA form (162 048 bytes) and for the 32-token tile (160 496); at D = 128 they take
    # 167 168 and 165 632 of the CU's 163 840, and the 8-token tile (140 864) serves every token count
    assert (_rvq(4097, 124, 256), _rvq(4097, 128, 256)) == (fc.RVQ_MFMA16, fc.RVQ_T8)
    assert (_rvq(19200, 124, 100), _rvq(19200, 128, 100)) == (fc.RVQ_T32, fc.RVQ_T8)
    assert (_rvq(256, 128, 256), _rvq(1024, 128, 256), _rvq(19200, 128, 256)) == (fc.RVQ_TOKEN, fc.RVQ_T8, fc.RVQ_T8)
    assert ops.rvq_ema_forward_kernel_name(109, 96, 75, 512) == fc.RVQ_MFMA32      # n = B * T


def test_dac_rvq_decision_boundaries():
    for C in (256, 512, 1024):
        assert (_dac(256, C), _dac(257, C)) == (fc.dac_form("lat1", C), fc.dac_form("lat2", C))
        assert (_dac(1024, C), _dac(1025, C)) == (fc.dac_form("lat2", C), fc.dac_form("tile", C))
        tile = fc.dac_form("tile", C)
        assert _dac(75, C, K=256) == tile and _dac(75, C, K=2048) == tile          # the latency forms are K = 1024 only ...
        assert _dac(75, C, prepared=False) == tile                                 # ... need the prepared codebook ...
        assert _dac(75, C, aligned=False) == tile and _dac(450, C, aligned=False) == tile      # ... and 16-byte aligned operands
    assert ops.dac_rvq_kernel_name(3, 1024, 99, 1024) == fc.dac_form("lat2", 1024)             # n = B * T
    from multimodal_vqvae_compression_audio_tactile_amd._lib import MvqError
    with pytest.raises(MvqError):
        ops.dac_rvq_kernel_name(1, 768, 75, 1024)                                  # no kernel is compiled for this width


# ------------------------------------------------------------------------------------------ the oracle against float64
def _torch_layernorm(v, gamma, beta, eps, do_tanh, post_scale):
    """The reference's arithmetic: torch's fp32 CPU layer_norm over the channel axis (then tanh and the scale, as TokenNorm)."""
    y = torch.nn.functional.layer_norm(torch.from_numpy(v.copy()).permute(0, 2, 1), (v.shape[1],), torch.from_numpy(gamma.copy()),
                                       torch.from_numpy(beta.copy()), eps)
    if do_tanh:
        y = torch.tanh(y)
    if do_tanh or post_scale != 1.0:
        y = torch.tensor(post_scale, dtype=torch.float32) * y
    return y.permute(0, 2, 1).numpy()


@pytest.mark.parametrize("case", fc.LN_CASES, ids=fc.ln_id)
def test_oracle_layernorm_against_float64(case, orc):
    """orc.layernorm_c (sequential fp32 sums in channel order, the contract every kernel form reproduces bit for bit) against a
    float64 restatement, at every LayerNorm case.  Tolerance per case: 8 x the largest error torch's own fp32 CPU layer_norm makes
    against float64 on the same input, floored at 1e-6.

    Measured, largest error of the oracle over that of torch, per width (smallest .. largest over the width's cases):
        C     8: 0.73 .. 1.62     C    24: 1.35     C    48: 1.08     C    64: 1.00 .. 1.40     C    72: 1.43 .. 1.99
        C   200: 1.00 .. 3.06     C  1024: 2.34 .. 4.80     C  1088: 3.46 .. 7.01     C  1152: 4.10     C  1216: 2.63
        C  1278: 2.95 .. 4.73     C  1279: 3.20 .. 4.41     C  1280: 4.03 .. 7.03
    The two ratios of 7 are cases of five tokens, where torch's largest error is a maximum over few values (1.8e-7 and 4.4e-7
    where its other cases of those widths show 4.7e-7 .. 9.0e-7); cases of 65 tokens or more stay at or below 4.4.  The figures are
    the same under torch's AVX-512 and AVX2 kernels; under its scalar kernels (ATEN_CPU_CAPABILITY=default) the largest is 5.7.

    Recorded, not asserted: with a mean of 30 standard deviations (x = 30 + N(0, 1), 256 tokens) the sequential order of the
    contract loses more than torch's pairwise moments do -- C = 8: 0.9 x, 72: 3.6 x, 200: 6.5 x, 1024: 12.8 x, 1280: 21.3 x,
    2050: 17.3 x torch's error (9.0e-5 against 4.2e-6 at C = 1280).  The model's LayerNorm inputs are zero-mean."""
    B, C, T, opts, _ = case
    i = fc.ln_inputs(case)
    eps, do_tanh, post_scale = fc.ln_params(opts)
    want = fc.ln_float64(i["v"], i["gamma"], i["beta"], eps, do_tanh, post_scale)
    err_torch = float(np.abs(_torch_layernorm(i["v"], i["gamma"], i["beta"], eps, do_tanh, post_scale) - want).max())
    err = float(np.abs(fc.oracle_result("ln", case, orc)[0] - want).max())
    tol = max(8.0 * err_torch, 1e-6)
    print(f"{fc.ln_id(case)}: oracle {err:.3e}, torch {err_torch:.3e}, ratio {err / err_torch:.2f}, tolerance {tol:.3e}")
    assert err <= tol


@pytest.mark.parametrize("case", [c for c in fc.RVQ_CASES if not c[6]], ids=fc.rvq_id)
def test_oracle_search_against_float64(case, orc):
    """orc.rvq_ema_forward's indices against a float64 arg-max of the same residual search, wherever the float64 top-two gap
    exceeds 1e-5 (fp32 round-off of these scores is below 1e-6).  The table's inputs are drawn so that EVERY search qualifies
    (smallest gap of the table: 1.88e-5): the share of tokens left out is 0, and that is asserted."""
    B, D, T, nb, K, use, _, _ = case
    z, books = fc.rvq_inputs(case)
    _, idx = fc.oracle_result("rvq", case, orc)
    want, gap = fc.rvq_float64(z, books, use)
    ok = gap > fc.RVQ_MIN_GAP
    left_out = float((~ok).mean())
    print(f"{fc.rvq_id(case)}: smallest float64 gap {gap.min():.3e}, share of tokens left out {left_out:.2e}")
    assert left_out == 0.0
    assert idx.shape == want.shape and np.array_equal(idx[ok], want[ok])


@pytest.mark.parametrize("case", [c for c in fc.RVQ_CASES if c[6]], ids=fc.rvq_id)
def test_oracle_search_ties_pick_the_lowest_index(case, orc):
    z, books = fc.rvq_inputs(case)
    assert all(np.array_equal(books[0, k], books[0, fc.TIE_CODES[0]]) for k in fc.TIE_CODES)
    assert fc.TIE_CODES[1] < 256 <= fc.TIE_CODES[2]                  # duplicates on both sides of a 256-code LDS pass
    _, idx = fc.oracle_result("rvq", case, orc)
    assert (idx == fc.TIE_CODES[0]).all()
