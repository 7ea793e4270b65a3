"""-m gpu: the PLC evaluation on the MI355X (csrc/mel_ssim.hip, plc.py) -- the mel SSIM kernel against the float64
restatement tests/plc_ref/ssim_ref.py, its width rules and determinism, the frame subsets, the masked mel ST-SIM against the
reference fixture G17, the subset statistics against G15 and evaluate_file (pass 1 of PLC/PLC1_eval.py:eval_model) against
G18 (tests/golden/make_golden_plc_stsim.py)."""
import math
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
import plc_eval_inputs as pe  # noqa: E402
import plc_inputs as pi  # noqa: E402
from plc_ref import ssim_ref as S  # noqa: E402

GOLD = ROOT / "tests" / "golden"
WIDTHS = (7, 8, 9, 13, 188, 751, 2251, 5626, 20481)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def plane(W, seed):
    """An un-normalised mel-like plane pair [64, 2W] (x columns 0..W-1, y columns W..2W-1) and its per-side maxima."""
    r = np.random.default_rng(seed)
    env = np.exp(-np.arange(64) / 20.0)[:, None]
    x = (env * r.gamma(0.6, 1.0, (64, W)) * 3.0).astype(np.float32)
    y = (x * r.uniform(0.7, 1.3, (64, W)) + 0.05 * r.gamma(0.5, 1.0, (64, W))).astype(np.float32)
    M = np.concatenate([x, y], axis=1)
    maxv = np.array([x.max(), y.max()], np.float32)
    return M, maxv


def images(M, maxv, W):
    """The normalised images the kernel sees: the same float32 true division."""
    d = np.maximum(maxv, np.float32(1e-8))
    return M[:, :W] / d[0], M[:, W:] / d[1]


def run(dev, M, maxv, descs, widths, max_width, cols=None, mode="ssim"):
    from multimodal_vqvae_compression_audio_tactile_amd import ops
    t = lambda a, dt: torch.as_tensor(np.asarray(a, dt)).to(dev)
    out = ops.mel_ssim(t(M, np.float32), t(maxv, np.float32), t(descs, np.int32), t(widths, np.int32), max_width,
                       cols=None if cols is None else t(cols, np.int32), mode=mode)
    return out.cpu().numpy()


@pytest.mark.parametrize("W", WIDTHS)
def test_ssim_kernel_matches_float64_restatement(dev, W):
    M, maxv = plane(W, 1000 + W)
    X, Y = images(M, maxv, W)
    got = run(dev, M, maxv, [[0, W, 0, 1, -1]], [W], W)[0]
    assert abs(got - S.structural_similarity(X, Y)) <= 1e-6, (got, S.structural_similarity(X, Y))


@pytest.mark.parametrize("W", (40, 751, 5626))
def test_ssim_kernel_on_compacted_subsets(dev, W):
    M, maxv = plane(W, 2000 + W)
    X, Y = images(M, maxv, W)
    r = np.random.default_rng(W)
    lists, descs, widths, off = [], [], [], 0
    for k in (7, 9, W // 3, W - 5):
        c = np.sort(r.choice(W, size=k, replace=False)).astype(np.int32)
        lists.append(c); descs.append([0, W, 0, 1, off]); widths.append(k); off += k
    got = run(dev, M, maxv, descs, widths, W, cols=np.concatenate(lists))
    for g, c in zip(got, lists):
        assert abs(g - S.structural_similarity(X[:, c], Y[:, c])) <= 1e-6


def test_narrow_widths_and_norm_mode(dev):
    W = 64
    M, maxv = plane(W, 3)
    X, Y = images(M, maxv, W)
    ws = list(range(0, 7)) + [7, 20, 64]
    descs = [[0, W, 0, 1, -1]] * len(ws)
    ss = run(dev, M, maxv, descs, ws, W, mode="ssim")
    nn = run(dev, M, maxv, descs, ws, W, mode="norm")
    assert math.isnan(ss[0]) and math.isnan(nn[0])
    for i, w in enumerate(ws[1:], 1):
        want_n = S.norm_sim(X[:, :w], Y[:, :w])
        assert abs(nn[i] - want_n) <= 1e-6, (w, nn[i], want_n)
        want_s = want_n if w < 7 else S.structural_similarity(X[:, :w], Y[:, :w])
        assert abs(ss[i] - want_s) <= 1e-6, (w, ss[i], want_s)


def test_bit_identical_run_to_run_and_in_any_batch(dev):
    W = 2251
    M, maxv = plane(W, 4)
    ws = [W, 3, 751, 0, 7, 1500, 20]
    descs = [[0, W, 0, 1, -1]] * len(ws)
    for mode in ("ssim", "norm"):
        a = run(dev, M, maxv, descs, ws, W, mode=mode)
        b = run(dev, M, maxv, descs, ws, W, mode=mode)
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
        perm = [4, 2, 0, 6, 1, 5, 3]
        c = run(dev, M, maxv, [descs[i] for i in perm], [ws[i] for i in perm], W, mode=mode)
        assert np.array_equal(c.view(np.uint64), a[perm].view(np.uint64))
        for i, w in enumerate(ws):
            alone = run(dev, M, maxv, [descs[i]], [w], W, mode=mode)
            assert np.array_equal(alone.view(np.uint64), a[i:i + 1].view(np.uint64)), (mode, w)


@pytest.mark.parametrize("name", list(pe.STSIM_CASES))
def test_frame_token_mask_equals_reference(dev, name):
    from multimodal_vqvae_compression_audio_tactile_amd import frame_token_mask, ops
    G17 = np.load(GOLD / "g17_plc_stsim.npz")
    T, L, _, _ = pe.STSIM_CASES[name]
    _, _, lm = pe.stsim_case(name)
    fm = frame_token_mask(torch.from_numpy(lm).to(dev), T)
    want = G17[f"{name}.frame_mask"]
    assert fm.is_cuda and np.array_equal(fm.cpu().numpy(), want)
    _, cols, counts = ops.frame_subsets(torch.from_numpy(lm).to(dev), T, want.size)
    n_m, n_u = counts.cpu().tolist()
    if L:
        assert (n_m, n_u) == (int(want.sum()), int((~want).sum()))
        c = cols.cpu().numpy()
        assert np.array_equal(c[0, :n_m], np.where(want)[0]) and np.array_equal(c[1, :n_u], np.where(~want)[0])
    else:
        assert (n_m, n_u) == (0, 0)


def close(got, want, tol):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    ok = ~np.isnan(want)
    assert np.all(np.abs(got[ok] - want[ok]) <= tol), (got, want)


@pytest.mark.parametrize("name", list(pe.STSIM_CASES))
def test_stsim_matches_reference_fixture(dev, name):
    from multimodal_vqvae_compression_audio_tactile_amd import stsim_mel_global, stsim_mel_with_mask
    G17 = np.load(GOLD / "g17_plc_stsim.npz")
    ref, est, lm = pe.stsim_case(name)
    r, e, m = (torch.from_numpy(x).to(dev) for x in (ref, est, lm))
    for backend in ("ssim", "norm"):
        close(stsim_mel_with_mask(r, e, m, backend=backend), G17[f"{name}.{backend}.with_mask"], 2e-5)
        close([stsim_mel_global(r, e, backend=backend)], [G17[f"{name}.{backend}.global"]], 2e-5)


def test_subset_stats_match_g15(dev):
    from multimodal_vqvae_compression_audio_tactile_amd import ops, plc
    G15 = np.load(GOLD / "g15_plc_metrics.npz")
    ref, est, masks = pi.metric_inputs()
    r, e = torch.from_numpy(ref).to(dev), torch.from_numpy(est).to(dev)
    keys = ("mae_masked", "mae_unmasked", "snr_masked_db", "snr_unmasked_db", "psnr_masked_db", "psnr_unmasked_db")
    for name, lm in masks.items():
        st = ops.subset_stats(r, e, torch.from_numpy(lm).to(dev)).cpu().tolist()
        sm = G15[f"{name}.sample_mask"]
        assert st[0] == sm.sum() and st[4] == (~sm).sum()
        row = plc._row_from(st, [0.0] * 3, ref.size, lm.size, pi.METRIC_PEAK, 0)
        for k, w in zip(keys, G15[f"{name}.values"]):
            if math.isnan(w):
                assert math.isnan(row[k]), (name, k)
            else:
                assert abs(row[k] - w) <= 1e-5 * max(1.0, abs(w)), (name, k, row[k], w)


@pytest.fixture(scope="module")
def net(dev):
    from multimodal_vqvae_compression_audio_tactile_amd import build_plc
    return build_plc(pi.plc_state(), device=dev)


@pytest.mark.parametrize("name", list(pe.EVAL_FILES))
def test_evaluate_file_matches_reference_rows(dev, net, name):
    from multimodal_vqvae_compression_audio_tactile_amd import evaluate_file, plc
    G18 = np.load(GOLD / "g18_plc_eval_rows.npz")
    a, t, lm = pe.eval_file(name)
    peak = float(G18["peak"])
    for backend in ("ssim", "norm"):
        row = evaluate_file(net, torch.from_numpy(a), 24000, torch.from_numpy(t), 24000, peak,
                            mask=torch.from_numpy(lm)[None].to(dev), backend=backend)
        want = dict(zip(plc.ROW_KEYS, G18[f"{name}.{backend}.row"]))
        assert row["best_shift"] == int(G18[f"{name}.best_shift"])
        assert row["len_samples"] == int(want["len_samples"])
        for k in ("psnr_global_db", "psnr_masked_db", "psnr_unmasked_db", "snr_masked_db", "snr_unmasked_db"):
            assert abs(row[k] - want[k]) <= 1e-4, (k, row[k], want[k])
        for k in ("mae_masked", "mae_unmasked"):
            assert abs(row[k] - want[k]) <= 1e-5 * abs(want[k]), (k, row[k], want[k])
        mg = float(G18[f"{name}.mae_global"])
        assert abs(row["mae_global"] - mg) <= 1e-5 * abs(mg)
        close([row[k] for k in ("stsim_global", "stsim_masked", "stsim_unmasked")],
              [want[k] for k in ("stsim_global", "stsim_masked", "stsim_unmasked")], 2e-5)


def test_bad_shapes_are_refused(dev):
    from multimodal_vqvae_compression_audio_tactile_amd import MvqError, ops
    W = 32769
    M = torch.zeros(64, 2 * W, device=dev)
    maxv = torch.ones(2, device=dev)
    desc = torch.tensor([[0, W, 0, 1, -1]], dtype=torch.int32, device=dev)
    widths = torch.tensor([W], dtype=torch.int32, device=dev)
    with pytest.raises(MvqError):
        ops.mel_ssim(M, maxv, desc, widths, W)
    with pytest.raises(MvqError):
        ops.mel_ssim(torch.zeros(63, 100, device=dev), maxv, desc, torch.tensor([50], dtype=torch.int32, device=dev), 50)
    with pytest.raises(MvqError):
        ops.frame_subsets(torch.zeros(10, dtype=torch.bool, device=dev), 10 * 320, W)
    from multimodal_vqvae_compression_audio_tactile_amd import _lib
    lib = _lib.lib()           # the C entry point refuses before any launch, whatever the pointers
    assert lib.mvq_mel_ssim_f32(None, 64, 100000, None, 2, None, None, 0, None, 1, 40000, 1, None, None) != 0
    assert lib.mvq_mel_ssim_f32(None, 63, 100, None, 2, None, None, 0, None, 1, 50, 1, None, None) != 0
    assert lib.mvq_frame_subsets(None, 10, 3200, 128, 40000, None, None, None, None, None) != 0


def test_thirty_second_file(dev, net):
    from multimodal_vqvae_compression_audio_tactile_amd import evaluate_file, plc, synth
    T = 30 * 24000
    a = synth.audio_segments(1, seed=301, T=T)[0]
    t = 0.8 * synth.tactile_segments(1, seed=301, T=T)[0]
    torch.manual_seed(5)
    row = evaluate_file(net, a, 24000, t, 24000, 1.0)
    assert set(plc.ROW_KEYS) <= set(row) and abs(row["best_shift"]) <= 400
    assert T - 400 <= row["len_samples"] <= T
    for k in plc.ROW_KEYS:
        assert math.isfinite(row[k]), (k, row[k])
