"""-m gpu: every kernel the LayerNorm, RVQ-EMA search and DAC residual-VQ launchers can choose, at the cases of
tests/forward_forms_cases.py, BIT-EXACT against the CPU oracle (tests/test_forward_forms_host.py holds the oracle against
float64 at the same inputs and the dispatch against the tables).  Every case asserts, through the launcher's own decision
function, that it ran the kernel it is listed under."""
import numpy as np
import pytest
import torch

import forward_forms_cases as fc

pytestmark = pytest.mark.gpu


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.array(a, copy=True)).to(dev)


def _aligned(*ts):
    return all(t is None or t.data_ptr() % 16 == 0 for t in ts)


@pytest.mark.parametrize("case", fc.LN_CASES, ids=fc.ln_id)
def test_layernorm_forms_bit_exact(case, orc, dev):
    from multimodal_vqvae_compression_audio_tactile_amd import ops
    B, C, T, opts, form = case
    assert ops.layernorm_kernel_name(B, C, T) == form
    i = fc.ln_inputs(case)
    eps, do_tanh, post_scale = fc.ln_params(opts)
    want, = fc.oracle_result("ln", case, orc)                # the oracle on (x - sub) + pe, formed in fp32 numpy in that order
    g, b, pe = _t(i["gamma"], dev), _t(i["beta"], dev), _t(i["pe"], dev)
    kw = dict(pe=pe, eps=eps, do_tanh=do_tanh, post_scale=post_scale)
    got = ops.layernorm_c(_t(i["x"], dev), g, b, sub=_t(i["sub"], dev), **kw).cpu().numpy()
    assert got.shape == want.shape and np.array_equal(got, want)
    if "folded" in opts:                                     # the token-folded [1, C, B*T] layout: same kernel, other strides
        sub = None if i["sub"] is None else _t(fc.fold(i["sub"]), dev)
        folded = ops.layernorm_c(_t(fc.fold(i["x"]), dev), g, b, sub=sub, folded_batch=B, **kw).cpu().numpy()
        assert folded.shape == (1, C, B * T)
        assert np.array_equal(fc.unfold(folded, B), got) and np.array_equal(fc.unfold(folded, B), want)


@pytest.mark.parametrize("case", fc.RVQ_CASES, ids=fc.rvq_id)
def test_rvq_search_forms_bit_exact(case, orc, dev):
    from multimodal_vqvae_compression_audio_tactile_amd import ops
    B, D, T, nb, K, use, tie, form = case
    z, books = fc.rvq_inputs(case)
    want_q, want_idx = fc.oracle_result("rvq", case, orc)
    zt, bt = _t(z, dev), _t(books, dev)
    assert ops.rvq_ema_forward_kernel_name(B, D, T, K, _aligned(bt)) == form
    q, idx = ops.rvq_ema_forward(zt, bt, use, return_indices=True)
    idx = idx.cpu().numpy()
    assert idx.shape == want_idx.shape == (nb if use is None else use, B * T)
    assert np.array_equal(idx, want_idx.astype(np.int64))
    assert np.array_equal(q.cpu().numpy(), want_q)
    if tie:                                                  # codes 17, 40, 300, 499 are one row and every token is that row
        assert (idx == fc.TIE_CODES[0]).all()


@pytest.mark.parametrize("case", fc.DAC_CASES, ids=fc.dac_id)
def test_dac_rvq_forms_bit_exact(case, orc, dev):
    from multimodal_vqvae_compression_audio_tactile_amd import ops
    B, C, T, nq, K, prepared, nq_item, kind = case
    sd, z, w = fc.dac_inputs(case)
    want_zq, want_codes, want_lat = fc.oracle_result("dac", case, orc)
    in_w, in_b, cb, out_w, out_b = (_t(w[k], dev) for k in ("in_w", "in_b", "cb", "out_w", "out_b"))
    prep = ops.dac_rvq_prepare(cb) if prepared else None
    assert ops.dac_rvq_kernel_name(B, C, T, K, prepared, _aligned(in_w, out_w, cb, prep[0] if prep else None)) == fc.dac_form(kind, C)
    items = None if nq_item is None else torch.tensor(nq_item, dtype=torch.int32, device=dev)
    zq, codes, lat = ops.dac_rvq(_t(z, dev), in_w, in_b, cb, out_w, out_b, nq, nq_item=items, prepared=prep)
    # include/mvq.h: codes / latents of all nq_use stages are produced, with or without nq_item
    assert np.array_equal(codes.cpu().numpy(), want_codes)
    assert np.array_equal(lat.cpu().numpy(), want_lat)
    zq = zq.cpu().numpy()
    if nq_item is None:
        assert np.array_equal(zq, want_zq)
    else:                                                    # ... and item b's z_q sums only its first nq_item[b] stages
        for b_i, n in enumerate(nq_item):
            assert np.array_equal(zq[b_i], orc.dac_quantizer(sd, z[b_i:b_i + 1], n)[0][0]), (b_i, n)
        assert not np.array_equal(zq, want_zq)
