"""-m gpu: packet-loss concealment on the MI355X -- the full-sequence attention kernels (forward bit-exact, backward against
float64), the masked fill, CrossPredictor over whole sequences, AllPredPLC.forward_step (inference and one training step) and the
masked / unmasked metrics, against the oracle, a long-sequence C restatement of orc_attention (tests/plc_ref) and the reference
fixtures G13-G15 (tests/golden/make_golden_plc.py)."""
import ctypes
import io
import math
import random
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
import plc_inputs as pi  # noqa: E402

GOLD = ROOT / "tests" / "golden"
TOL, WORST = 2e-4, 2e-5          # the bars of tests/test_gpu_train_shapes.py: whole tensor, worst token


def rel(got, want):
    got = torch.as_tensor(got).detach().double().cpu().reshape(-1); want = torch.as_tensor(want).detach().double().cpu().reshape(-1)
    return float((got - want).norm() / want.norm().clamp_min(1e-30))


def worst_token(got, want):
    """Largest relative L2 error over tokens (columns) of [B, C, T] tensors."""
    g = got.detach().double().cpu().permute(1, 0, 2).reshape(got.shape[1], -1)
    w = want.detach().double().cpu().permute(1, 0, 2).reshape(want.shape[1], -1)
    return float(((g - w).norm(dim=0) / w.norm(dim=0).clamp_min(1e-30)).max())


def fold(x):
    B, C, T = x.shape
    return x.permute(1, 0, 2).reshape(1, C, B * T).contiguous()


def unfold(x, B):
    C = x.shape[1]
    return x.reshape(C, B, -1).permute(1, 0, 2).contiguous()


@pytest.fixture(scope="session")
def attref(tmp_path_factory):
    """tests/plc_ref/attention_seq_ref.c built with the oracle's flags (oracle/c/Makefile) into a temporary directory."""
    out = tmp_path_factory.mktemp("plc_ref") / "libattref.so"
    subprocess.run(["gcc", "-O3", "-mavx2", "-mfma", "-ffp-contract=off", "-fno-math-errno", "-fopenmp", "-fPIC", "-Wall",
                    "-Wno-unknown-pragmas", f"-I{ROOT / 'oracle' / 'c'}", "-shared", "-o", str(out),
                    str(ROOT / "tests" / "plc_ref" / "attention_seq_ref.c"), "-lm"], check=True, capture_output=True)
    lib = ctypes.CDLL(str(out))
    fp = ctypes.POINTER(ctypes.c_float)
    lib.ref_attention_seq.argtypes = [fp] * 4 + [ctypes.c_int] * 5
    lib.ref_attention_seq.restype = ctypes.c_int

    def run(Q, K, V, heads):
        Q, K, V = (np.ascontiguousarray(x, np.float32) for x in (Q, K, V))
        B, C, Tq = Q.shape
        ctx = np.zeros_like(Q)
        p = lambda a: a.ctypes.data_as(fp)
        assert lib.ref_attention_seq(p(Q), p(K), p(V), p(ctx), B, heads, C // heads, Tq, K.shape[2]) == 0
        return ctx
    return run


def _qkv(B, C, Tq, Tk, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, C, Tq, generator=g), torch.randn(B, C, Tk, generator=g), torch.randn(B, C, Tk, generator=g))


# ------------------------------------------------------------------------------------------------------------ forward kernel
CHUNK_SHAPES = [(16, 3, 16, 16), (16, 2, 64, 64), (16, 1, 1, 64), (16, 2, 64, 1), (16, 1, 37, 0), (128, 3, 16, 16),
                (128, 2, 11, 16), (128, 1, 16, 9), (128, 2, 28, 28), (128, 1, 5, 0)]


@pytest.mark.parametrize("dh,B,Tq,Tk", CHUNK_SHAPES)
@pytest.mark.parametrize("folded", [False, True])
def test_attention_seq_bit_equal_to_chunk_kernel(dh, B, Tq, Tk, folded, dev):
    """On every shape mvq_attention_f32 accepts, the full-sequence kernel gives the same bits (the predictor routing of existing
    paths depends on it): dh 16 and 128, contiguous and token-folded, Tk = 0, Tq != Tk."""
    from multimodal_vqvae_compression_audio_tactile_amd import ops
    H = 8
    assert ops.attention_fits(dh, Tq, Tk)
    q, k, v = (x.to(dev) for x in _qkv(B, H * dh, Tq, Tk, seed=dh * 1000 + Tq * 10 + Tk))
    if folded:
        q, k, v = fold(q), fold(k), fold(v)
    fb = B if folded else None
    want = ops.attention(q, k, v, H, folded_batch=fb)
    got = ops.attention_seq(q, k, v, H, folded_batch=fb)
    assert torch.equal(got, want)
    if Tk == 0:
        assert not got.any()


LONG_SHAPES = [(2, 75, 75), (1, 225, 225), (2, 1, 300), (1, 300, 1), (1, 32, 2000), (1, 16, 8192)]


@pytest.mark.parametrize("B,Tq,Tk", LONG_SHAPES)
def test_attention_seq_bit_equal_to_long_restatement(B, Tq, Tk, attref, dev):
    """Beyond the chunk kernel's 64 tokens: bit-equal to the C restatement of orc_attention's loop (tests/plc_ref), and within
    fp32 round-off of float64 torch."""
    from multimodal_vqvae_compression_audio_tactile_amd import ops
    H, dh = 8, 128
    q, k, v = _qkv(B, H * dh, Tq, Tk, seed=Tq * 7 + Tk)
    got = ops.attention_seq(q.to(dev), k.to(dev), v.to(dev), H).cpu()
    want = attref(q.numpy(), k.numpy(), v.numpy(), H)
    assert np.array_equal(got.numpy(), want)
    sp = lambda x: x.double().reshape(B, H, dh, -1)
    att = torch.einsum("bhdi,bhdj->bhij", sp(q), sp(k)) / math.sqrt(dh)
    ref64 = torch.einsum("bhij,bhdj->bhdi", att.softmax(-1), sp(v)).reshape(B, H * dh, Tq)
    r = rel(got, ref64)
    print(f"attention_seq B={B} Tq={Tq} Tk={Tk}: relative error vs float64 {r:.2e}")
    assert r < 1e-5


def test_attention_seq_refuses_oversize_before_launch(dev):
    from multimodal_vqvae_compression_audio_tactile_amd import ops
    from multimodal_vqvae_compression_audio_tactile_amd._lib import MvqError
    q = torch.randn(1, 128, 8193, device=dev)
    k = torch.randn(1, 128, 16, device=dev)
    with pytest.raises(MvqError):
        ops.attention_seq(q, k, k, 8)
    with pytest.raises(MvqError):
        ops.attention_seq(k, q, q, 8)
    with pytest.raises(MvqError):
        ops.attention_seq_bwd(k[..., :16], q[..., :513].contiguous(), q[..., :513].contiguous(), k[..., :16], 8)
    torch.cuda.synchronize()
    assert torch.isfinite(ops.attention_seq(k, k, k, 8)).all()          # the stream is clean


# ----------------------------------------------------------------------------------------------------------- backward kernel
@pytest.mark.parametrize("B", [1, 6])
@pytest.mark.parametrize("T", [75, 150, 300])
def test_attention_seq_backward_against_float64(B, T, dev):
    """gq, gk, gv of the full-sequence backward (token-folded, as the training step calls it) against float64 autograd: the
    suite's bars, relative L2 <= 2e-4 per tensor and <= 2e-5 for the worst token."""
    from multimodal_vqvae_compression_audio_tactile_amd import ops
    H, dh = 8, 128
    g = torch.Generator().manual_seed(B * 1000 + T)
    q, k, v, go = (torch.randn(B, H * dh, T, generator=g, dtype=torch.float64) for _ in range(4))
    qr, kr, vr = (x.clone().requires_grad_(True) for x in (q, k, v))
    sp = lambda x: x.reshape(B, H, dh, T)
    att = torch.einsum("bhdi,bhdj->bhij", sp(qr), sp(kr)) / math.sqrt(dh)
    ctx = torch.einsum("bhij,bhdj->bhdi", att.softmax(-1), sp(vr)).reshape(B, H * dh, T)
    (ctx * go).sum().backward()
    got = ops.attention_seq_bwd(*(fold(x.float()).to(dev) for x in (q, k, v, go)), H, folded_batch=B)
    torch.cuda.synchronize()
    figures = []
    for name, gt, want in zip(("gq", "gk", "gv"), got, (qr.grad, kr.grad, vr.grad)):
        gt = unfold(gt.cpu(), B)
        assert torch.isfinite(gt).all(), name
        r, w = rel(gt, want), worst_token(gt, want)
        figures.append(f"{name} {r:.2e} / worst token {w:.2e}")
        assert r <= TOL and w <= WORST, (name, r, w)
    print(f"attention_seq_bwd B={B} T={T}: " + ", ".join(figures))


# ------------------------------------------------------------------------------------------------------------------- predictor
def _predict_module(dev):
    from multimodal_vqvae_compression_audio_tactile_amd import CrossPredictor
    sd = pi.plc_state()
    cp = CrossPredictor(1024)
    cp.load_state_dict({k[len("predict."):]: v for k, v in sd.items() if k.startswith("predict.")}, strict=True)
    return cp.to(dev).eval(), {k: v.numpy() for k, v in sd.items()}


def oracle_predictor(orc, attref, sd, zt, za, heads=8, P="predict."):
    """oracle.cross_predictor with the attention swapped for the long-sequence restatement (orc_attention stops at 64 keys)."""
    pe = np.asarray(sd[P + "pos.pe"], np.float32)
    Tq, Tk = zt.shape[2], za.shape[2]
    q = orc.layernorm_c(zt + pe[:Tq].T[None], sd[P + "ln_q.weight"], sd[P + "ln_q.bias"])
    kv = orc.layernorm_c(za + pe[:Tk].T[None], sd[P + "ln_kv.weight"], sd[P + "ln_kv.bias"])
    Q = orc._linear(q, sd[P + "q_proj.weight"])
    K = orc._linear(kv, sd[P + "k_proj.weight"])
    V = orc._linear(kv, sd[P + "v_proj.weight"])
    ctx = attref(Q, K, V, heads)
    y1 = orc._linear(ctx, sd[P + "out.weight"], residual=q)
    h = orc.layernorm_c(y1, sd[P + "ffn.0.weight"], sd[P + "ffn.0.bias"])
    h = orc.gelu(orc._linear(h, sd[P + "ffn.1.weight"], sd[P + "ffn.1.bias"]))
    return orc._linear(h, sd[P + "ffn.3.weight"], sd[P + "ffn.3.bias"], residual=y1)


@pytest.mark.parametrize("name", list(pi.PRED_CASES))
def test_predictor_over_whole_sequences(name, orc, attref, dev):
    """CrossPredictor(zt, qa) at T = 75 and 300 (the chunk attention refuses both): bit-exact against the oracle composition
    with the long attention, and within fp32 round-off of the reference's values (G13)."""
    B, T, seed = pi.PRED_CASES[name]
    cp, sd = _predict_module(dev)
    zt, qa = pi.pred_inputs(B, T, seed)
    with torch.no_grad():
        got = cp(torch.from_numpy(zt).to(dev), torch.from_numpy(qa).to(dev)).cpu()
    assert got.shape == (B, 1024, T)
    assert np.array_equal(got.numpy(), oracle_predictor(orc, attref, sd, zt, qa))
    ref = np.load(GOLD / "g13_plc_forward.npz")[f"pred.{name}"]
    r = rel(got.reshape(-1)[::pi.LAT_STRIDE], ref)
    print(f"predictor {name}: relative error vs reference {r:.2e}")
    assert r <= 1e-5


# ------------------------------------------------------------------------------------------------------------------------ fill
@pytest.mark.parametrize("folded", [False, True])
def test_mask_fill_is_the_torch_expression(folded, dev):
    """zt_in = zt * ~mask and z_filled = where(mask, z_pred, zt_in), bit for bit, with NaN, +-inf and -0 in both inputs; the
    backward equals torch autograd's gradient w.r.t. z_pred."""
    from multimodal_vqvae_compression_audio_tactile_amd import ops, train
    B, C, T = 3, 64, 75
    g = torch.Generator().manual_seed(5)
    zt, zp = torch.randn(B, C, T, generator=g), torch.randn(B, C, T, generator=g)
    for x in (zt, zp):
        x[0, 1, :7] = float("nan"); x[1, 2, 3:9] = float("inf"); x[2, 3, 10:20] = -float("inf"); x[0, 4, :] = -0.0
    mask = torch.rand(B, T, generator=g) < 0.5
    zt, zp, m = zt.to(dev), zp.to(dev), mask.to(dev)
    want_in = zt * (~m.unsqueeze(1))
    want_f = torch.where(m.unsqueeze(1), zp, want_in)
    a, b = (fold(zt), fold(zp)) if folded else (zt, zp)
    zt_in, zf = ops.plc_mask_fill(a, b, m, folded_batch=B if folded else None)
    if folded:
        zt_in, zf = unfold(zt_in, B), unfold(zf, B)
    bits = lambda x: x.cpu().view(torch.int32)
    assert torch.equal(bits(zt_in), bits(want_in)) and torch.equal(bits(zf), bits(want_f))
    neg = (zt < 0) & m.unsqueeze(1)
    assert neg.any() and torch.signbit(zt_in[neg]).all()                                    # a masked negative gives -0
    zpr = zp.clone().requires_grad_(True)
    gy = torch.randn(B, C, T, generator=g).to(dev)
    torch.where(m.unsqueeze(1), zpr, want_in).backward(gy)
    gz = ops.plc_mask_fill_bwd(fold(gy) if folded else gy, m, folded_batch=B if folded else None)
    gz = unfold(gz, B) if folded else gz
    assert torch.equal(bits(gz), bits(zpr.grad))
    zr = zp.clone().requires_grad_(True)
    out = train.PlcFill.apply(zt, zr, m, None)
    assert torch.equal(bits(out), bits(want_f))
    out.backward(gy)
    assert torch.equal(bits(zr.grad), bits(zpr.grad))


# -------------------------------------------------------------------------------------------------------- whole model, eval
def _np_state(sd):
    return {k: v.numpy() for k, v in sd.items()}


@pytest.mark.parametrize("name", list(pi.FWD_CASES))
def test_forward_step_inference_matches_oracle_and_reference(name, orc, attref, dev):
    """AllPredPLC.forward_step under no_grad with G13's mask: y_hat bit-exact against the oracle composition (backbones from
    oracle/oracle.py, predictor with the long attention) and within fp32 round-off of the reference's y_hat."""
    from multimodal_vqvae_compression_audio_tactile_amd import build_plc
    B, Tw, seed = pi.FWD_CASES[name]
    G13 = np.load(GOLD / "g13_plc_forward.npz")
    sd = pi.plc_state()
    net = build_plc(sd, device=dev)
    a, t = pi.waves(B, Tw, seed)
    mask = torch.from_numpy(G13[f"{name}.mask"])
    with torch.no_grad():
        out = net.forward_step(a.to(dev), t.to(dev), mask=mask.to(dev))
    assert torch.equal(out["latent_mask"][:, 0].cpu(), mask)
    y = out["y_hat"].cpu().numpy()
    s = _np_state(sd)
    qa = orc.dac_quantizer(s, orc.dac_encoder(s, a.numpy(), prefix="A_ENC."), prefix="A_QUANT.")[0]
    zt = orc.dac_encoder(s, t.numpy(), prefix="T_ENC.")
    keep = ~mask.numpy()[:, None, :]
    zt_in = zt * keep.astype(np.float32)
    zp = oracle_predictor(orc, attref, s, zt_in, qa)
    zf = np.where(~keep, zp, zt_in)
    want = orc.dac_decoder(s, zf, prefix="T_DEC.")
    Tm = min(want.shape[-1], Tw)
    want = np.nan_to_num(want[..., :Tm], nan=0.0, posinf=0.0, neginf=0.0)
    assert y.shape == want.shape == G13[f"{name}.y_hat"].shape
    assert np.array_equal(y, want)
    np.testing.assert_allclose(y, G13[f"{name}.y_hat"], rtol=0, atol=3e-5)
    assert rel(zp.reshape(-1)[::pi.LAT_STRIDE], G13[f"{name}.z_pred"]) <= 1e-5


def test_subset_metrics_match_reference(dev):
    from multimodal_vqvae_compression_audio_tactile_amd import masked_metrics, token_to_sample_mask
    G15 = np.load(GOLD / "g15_plc_metrics.npz")
    ref, est, masks = pi.metric_inputs()
    r, e = torch.from_numpy(ref).to(dev), torch.from_numpy(est).to(dev)
    keys = ("mae_masked", "mae_unmasked", "snr_masked", "snr_unmasked", "psnr_masked", "psnr_unmasked")
    for name, lm in masks.items():
        sm = token_to_sample_mask(torch.from_numpy(lm).to(dev), ref.size)
        assert sm.is_cuda and np.array_equal(sm.cpu().numpy(), G15[f"{name}.sample_mask"]), name
        got = masked_metrics(r, e, torch.from_numpy(lm).to(dev), pi.METRIC_PEAK)
        want = G15[f"{name}.values"]
        for k, w in zip(keys, want):
            if math.isnan(w):
                assert math.isnan(got[k]), (name, k)
            else:
                assert abs(got[k] - w) <= 1e-5 * max(1.0, abs(w)), (name, k, got[k], w)
    assert sum(math.isnan(x) for x in G15["all.values"]) == 3 and sum(math.isnan(x) for x in G15["none.values"]) == 3


# ---------------------------------------------------------------------------------------------------------- training step
def test_training_step_matches_reference_fixture(dev):
    """One PLC1.py training step on the HIP path (forward_step -> TrainingLoss -> backward) against G14, with the acceptance rule
    of tests/test_gpu_train.py: HIP error vs the float64 step <= max(1.5 x the reference's own fp32 error, floor).  Exactly the
    predict.* tensors get gradients; then clip 3.0, AdamW and a second, finite loss."""
    from multimodal_vqvae_compression_audio_tactile_amd import TrainingLoss, build_plc
    G14 = np.load(GOLD / "g14_plc_train_step.npz")
    B, Tw, seed = pi.TRAIN_CASE
    net = build_plc(pi.plc_state(), device=dev)                          # eval(): dropout off, as the fixture
    a, t = pi.waves(B, Tw, seed)
    a, t = a.to(dev), t.to(dev)
    mask = torch.from_numpy(G14["mask"]).to(dev)
    crit = TrainingLoss()
    out = net.forward_step(a, t, mask=mask)
    total = crit(out["y_hat"], out["tgt"])
    total.backward()
    got = np.array([float(crit.parts[k]) for k in ("l1", "stft", "mel")] + [float(total)])
    exact, ref = G14["f64.losses"], G14["losses"]
    err_hip, err_ref = np.abs(got - exact) / exact, np.abs(ref - exact) / exact
    print("PLC loss rel. error vs float64  HIP:", err_hip, " reference fp32:", err_ref)
    assert np.all(err_hip <= np.maximum(1.5 * err_ref, 2e-6)), (got, ref, exact)
    n, worst_hip, worst_ref = 0, 0.0, 0.0
    for name, p in net.named_parameters():
        if f"norm.{name}" not in G14.files:
            assert p.grad is None, name
            continue
        assert name.startswith("predict.") and p.grad is not None, name
        ex_n, ref_n = float(G14[f"f64.norm.{name}"]), float(G14[f"norm.{name}"])
        e_hip_n, e_ref_n = abs(float(p.grad.norm()) - ex_n) / ex_n, abs(ref_n - ex_n) / ex_n
        assert e_hip_n <= max(1.5 * e_ref_n, 2e-5), (name, e_hip_n, e_ref_n)
        sub = p.grad.reshape(-1)[::pi.GRAD_STRIDE].cpu().double()
        ex, rf = torch.from_numpy(G14[f"f64.sub.{name}"]), torch.from_numpy(G14[f"sub.{name}"]).double()
        e_hip, e_ref = rel(sub, ex), rel(rf, ex)
        assert e_hip <= max(1.5 * e_ref, 2e-5), (name, e_hip, e_ref)
        worst_hip, worst_ref = max(worst_hip, e_hip), max(worst_ref, e_ref)
        n += 1
    print(f"PLC sampled gradients over {n} tensors, worst relative error vs float64: HIP {worst_hip:.2e}, reference fp32 {worst_ref:.2e}")
    assert n == len([k for k in G14.files if k.startswith("norm.")]) == 14
    assert net.tokennorm.ln.weight.grad is None and net.tokennorm.ln.bias.grad is None
    params = [p for p in net.parameters() if p.requires_grad]
    opt = torch.optim.AdamW(params, lr=2e-4, weight_decay=1e-5)
    gn = torch.nn.utils.clip_grad_norm_(params, 3.0)
    assert torch.isfinite(gn)
    opt.step()
    opt.zero_grad(set_to_none=True)
    net.train()                                                           # ctx dropout on, as in PLC1.py's loop
    out2 = net.forward_step(a, t, mask=mask)
    total2 = crit(out2["y_hat"], out2["tgt"])
    assert torch.isfinite(total2) and float(total2) != float(total)
    total2.backward()
    assert all(torch.isfinite(p.grad).all() for p in net.predict.parameters() if p.requires_grad)


# ------------------------------------------------------------------------------------------------------- mask and checkpoint
def test_mask_generation_mask_fn_and_checkpoint(dev):
    from multimodal_vqvae_compression_audio_tactile_amd import build_plc, make_token_loss_mask
    for B, T_lat in ((6, 75), (1, 225), (2, 8)):
        gen_seed = 1234 + T_lat
        torch.cuda.manual_seed(gen_seed)
        got = make_token_loss_mask(B, T_lat, 2, 0.5, dev)
        torch.cuda.manual_seed(gen_seed)                                # the reference's steps: ONE rand(B, P), expand, pad
        P = max(1, T_lat // 2)
        lost = torch.rand(B, P, device=dev) < 0.5
        want = torch.zeros(B, T_lat, dtype=torch.bool, device=dev)
        n = min(T_lat, 2 * P)
        want[:, :n] = lost.unsqueeze(-1).expand(B, P, 2).reshape(B, -1)[:, :n]
        assert got.device.type == "cuda" and torch.equal(got, want)
    net = build_plc(pi.plc_state(), device=dev)
    a, t = pi.waves(2, 24000, 17)
    rng = random.Random(3)

    def bursts(batch_size, T_lat, device):                              # category-style bursts (PLC1_low_mid_high.py shape)
        m = torch.zeros(batch_size, T_lat, dtype=torch.bool)
        for b in range(batch_size):
            for _ in range(rng.randint(1, 3)):
                L = rng.randint(2, 20)
                s = rng.randint(0, T_lat - L)
                m[b, s:s + L] = True
        return m.to(device)
    with torch.no_grad():
        out = net.forward_step(a.to(dev), t.to(dev), mask_fn=bursts)
        out_default = net.forward_step(a.to(dev), t.to(dev))
    assert out["latent_mask"].shape == (2, 1, 75) and out["latent_mask"].any()
    assert torch.isfinite(out["y_hat"]).all() and out["y_hat"].shape == out["tgt"].shape == (2, 1, 23992)
    assert out_default["latent_mask"].shape == (2, 1, 75)
    buf = io.BytesIO()
    torch.save({"model": net.state_dict()}, buf)
    buf.seek(0)
    ckpt = torch.load(buf, map_location=dev)
    net2 = build_plc(device=dev)
    res = net2.load_state_dict(ckpt["model"], strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    m = out["latent_mask"][:, 0]
    with torch.no_grad():
        y1 = net.forward_step(a.to(dev), t.to(dev), mask=m)["y_hat"]
        y2 = net2.forward_step(a.to(dev), t.to(dev), mask=m)["y_hat"]
    assert torch.equal(y1, y2)


def test_long_file_inference_runs_on_the_seq_kernels(dev):
    """A whole 30-s file at B = 1 (T_lat = 2250): the predictor's attention runs over all tokens in one call."""
    from multimodal_vqvae_compression_audio_tactile_amd import build_plc
    net = build_plc(pi.plc_state(), device=dev)
    a, t = pi.waves(1, 24000 * 30, 19)
    with torch.no_grad():
        out = net.forward_step(a.to(dev), t.to(dev))
    assert out["latent_mask"].shape == (1, 1, 2250) and torch.isfinite(out["y_hat"]).all()
