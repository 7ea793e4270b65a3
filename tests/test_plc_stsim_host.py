"""CPU: the ST-SIM restatement (tests/plc_ref/ssim_ref.py) against the reference fixture G17
(tests/golden/make_golden_plc_stsim.py): float32 within 1e-6 of float64 on the reference's mel images, and the restatement run
through the host glue (float64 frame -> token rule, concatenated subsets, the < 7 fall-through) reproducing G17 in both
branches."""
import math
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
import plc_eval_inputs as pe  # noqa: E402
from plc_ref import ssim_ref as S  # noqa: E402

G17 = np.load(ROOT / "tests" / "golden" / "g17_plc_stsim.npz")


def same(got, want, tol):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    ok = ~np.isnan(want)
    assert np.all(np.abs(got[ok] - want[ok]) <= tol), (got, want)


@pytest.mark.parametrize("name", list(pe.STSIM_CASES))
def test_float32_restatement_is_within_1e6_of_float64(name):
    X, Y, fm = G17[f"{name}.X"], G17[f"{name}.Y"], G17[f"{name}.frame_mask"]
    images = [(X, Y)] + [(X[:, m], Y[:, m]) for m in (fm, ~fm) if m.sum() >= S.WIN]
    for A, B in images:
        assert abs(S.ssim_f32(A, B) - S.structural_similarity(A, B)) <= 1e-6


@pytest.mark.parametrize("name", list(pe.STSIM_CASES))
def test_host_glue_reproduces_reference(name):
    T, L, _, _ = pe.STSIM_CASES[name]
    _, _, lm = pe.stsim_case(name)
    X, Y = G17[f"{name}.X"], G17[f"{name}.Y"]
    assert np.array_equal(S.frame_mask(lm, T, X.shape[1]), G17[f"{name}.frame_mask"])
    for backend in ("ssim", "norm"):
        got = S.stsim_with_mask(X, Y, lm, T, backend, ssim=S.ssim_f32)
        same(got, G17[f"{name}.{backend}.with_mask"], 1e-6)
        same([S.stsim_core(X, Y, backend, S.ssim_f32)], [G17[f"{name}.{backend}.global"]], 1e-6)


def test_fixture_covers_the_rules():
    """NaN on empty sides and T_lat = 0; the norm fall-through below 7 frames differs from no fall-through."""
    nan = lambda n, b: [math.isnan(v) for v in G17[f"{n}.{b}.with_mask"]]
    assert nan("all", "ssim") == [False, False, True] and nan("none", "ssim") == [False, True, False]
    assert nan("tlat0", "ssim") == [False, True, True]
    for name, side in (("m3", 1), ("m6", 1), ("u2", 2)):
        X, Y, fm = G17[f"{name}.X"], G17[f"{name}.Y"], G17[f"{name}.frame_mask"]
        m = fm if side == 1 else ~fm
        assert 1 <= m.sum() < S.WIN
        assert G17[f"{name}.ssim.with_mask"][side] == G17[f"{name}.norm.with_mask"][side]
        assert abs(G17[f"{name}.ssim.with_mask"][side] - S.norm_sim(X[:, m], Y[:, m])) <= 1e-6
    assert G17["m7.frame_mask"].sum() == S.WIN
    assert G17["m7.ssim.with_mask"][1] != G17["m7.norm.with_mask"][1]
