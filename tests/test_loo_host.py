"""PSIS-LOO (d3p_amd.criteria.loo, d3p_psis_loo), host side: tests/psis_ref.py against ground truth and on its edge cases, the
calibration of its float64 term, the module surface and the C entry's declaration, every refusal of loo / posterior_loo / compare
before a device is touched, and compare on hand-made CPU results."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import psis_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def no_device(monkeypatch):
    import d3p_amd._lib as L

    def refuse(*a, **k):
        raise AssertionError("criteria reached require_device")
    monkeypatch.setattr(L, "require_device", refuse)


# ------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("k", [0.5, 0.9])
def test_reference_recovers_the_shape_of_generalised_pareto_ratios(k):
    """Importance ratios r with r - 1 ~ GPD(shape k, scale 1), columns of -log r, n = 4096, 200 columns: the mean k-hat is within
    0.05 of k (recorded: 0.502 and 0.880, sd 0.11 and 0.13, so the standard error of the mean is below 0.01)."""
    r = np.random.default_rng(5 + int(10 * k))
    ks = []
    for _ in range(200):
        g = ((1.0 - r.random(4096)) ** -k - 1.0) / k
        out = PR.psis_column((-np.log1p(g)).astype(np.float32))
        assert out["T"] == PR.tail_len(4096) == 192 and np.isfinite(out["elpd"])
        ks.append(out["k"])
    print(f"k = {k}: mean k-hat {np.mean(ks):.4f}, sd {np.std(ks):.4f}")
    assert abs(np.mean(ks) - k) <= 0.05


def test_tail_length_at_its_edges():
    assert [PR.tail_len(n) for n in (1, 5, 6, 20, 21, 225, 226, 65535)] == [1, 1, 2, 4, 5, 45, 46, 768]


def test_short_tails_keep_the_raw_ratios():
    r = np.random.default_rng(1)
    for n in (1, 2, 5, 6, 20):
        col = r.normal(-2.0, 1.0, n).astype(np.float32)
        out = PR.psis_column(col)
        assert out["k"] == np.inf and out["T"] <= 4, n
        # raw importance sampling: elpd = -log mean exp(-ll)
        raw = -(np.log(np.mean(np.exp(-(col.astype(np.float64) - col.min())))) - col.min())
        assert abs(out["elpd"] - raw) <= 1e-13 * max(1.0, abs(raw)), n
    out = PR.psis_column(r.normal(-2.0, 1.0, 21).astype(np.float32))
    assert out["T"] == 5 and np.isfinite(out["k"])                     # the smallest n with a fit


def test_equal_draws_and_ties_at_the_cut():
    out = PR.psis_column(np.full(130, -1.25, np.float32))
    assert out["elpd"] == -1.25 and out["lppd"] == -1.25 and out["k"] == np.inf and out["T"] == 0
    # 10 distinct values x 10: M = 20, the 21st largest x equals the 20th .. 30th, so the tail is the two top groups' worth less the tie
    col = np.repeat(np.arange(10, dtype=np.float32), 10) * -0.5
    out = PR.psis_column(col)
    assert out["T"] == 20 and np.array_equal(out["tail"], col < -3.75) and np.isfinite(out["k"])
    col[0] = -3.75                                                     # (now 11 at the third value from below: still T = 20)
    assert PR.psis_column(col)["T"] == 20


def test_special_values():
    base = np.random.default_rng(2).normal(-1.0, 0.5, 64).astype(np.float32)
    col = base.copy()
    col[7] = -np.inf
    out = PR.psis_column(col)
    assert out["elpd"] == -np.inf and out["k"] == np.inf and np.isfinite(out["lppd"])
    keep = np.delete(base, 7).astype(np.float64)
    assert abs(out["lppd"] - (np.log(np.exp(keep).sum()) - math.log(64))) <= 1e-13
    out = PR.psis_column(np.full(64, -np.inf, np.float32))
    assert out["elpd"] == -np.inf and out["k"] == np.inf and out["lppd"] == -np.inf
    col = base.copy()
    col[3] = np.nan
    col[4] = -np.inf
    out = PR.psis_column(col)
    assert np.isnan(out["elpd"]) and np.isnan(out["lppd"]) and np.isnan(out["k"])
    col = base.copy()
    col[3] = np.inf
    out = PR.psis_column(col)
    assert np.isnan(out["elpd"]) and np.isnan(out["k"]) and out["lppd"] == np.inf


def test_a_cut_below_log_dbl_min_is_raised_to_it():
    col = PR.low_cut_column()
    x = -col.astype(np.float64) - np.max(-col.astype(np.float64))
    M = PR.tail_len(col.size)
    assert np.sort(x)[::-1][M] < PR.LOG_DBL_MIN
    out = PR.psis_column(col)
    assert np.array_equal(out["tail"], x > PR.LOG_DBL_MIN) and 4 < out["T"] < M and np.isfinite(out["elpd"])
    fixed = PR.fixed_columns()
    got = {name: PR.psis_column(fixed[:, c]) for c, name in enumerate(PR.FIXED_NAMES)}
    assert got["ties"]["T"] == 20 and got["equal"]["T"] == 0 and got["low_cut"]["T"] == 8 and got["plain"]["T"] == 20
    assert got["equal"]["elpd"] == -1.25 and got["one_neg_inf"]["elpd"] == -np.inf and np.isnan(got["one_nan"]["lppd"])




# ------------------------------------------------------------------------------------------------ calibration
def test_the_float64_term_covers_the_perturbed_kernel_order_restatement():
    """Two columns of every matrix of the sweep, one perturbation seed: the deviations stay at or below the ones recorded over the
    whole sweep (the constants are 4 times those), and the tail and the k = +inf rows agree exactly (asserted inside calibrate)."""
    worst = PR.calibrate(PR.sweep_columns(2), seeds=(0,))
    print(worst)
    assert 0.0 < max(worst["elpd"].values()) <= PR.F64_ELPD / 4 and 0.0 < max(worst["lppd"].values()) <= PR.F64_LPPD / 4
    assert 0.0 < max(worst["k"].values()) * 2.0 ** -52 <= PR.F64_K_PER_COND / 4
    # the bound is dominated by the float32 rounding wherever the fit is well conditioned
    e, lp, k = PR.bounds(np.array([-3.0]), np.array([-2.0]), np.array([0.4]), np.array([50.0]))
    assert e[0] < 1.01 * 2.0 ** -24 * 3.0 and k[0] < 1.01 * 2.0 ** -24 * 0.4


def test_kernel_order_restatement_without_perturbation_is_the_reference_up_to_rounding():
    for kind, n, col in PR.sweep_columns(1):
        ref, got = PR.psis_column(col), PR.psis_column(col, kernel_order=True)
        assert got["T"] == ref["T"] and np.array_equal(got["tail"], ref["tail"])
        for name in ("elpd", "lppd"):
            assert abs(got[name] - ref[name]) <= PR.F64_ELPD * max(1.0, abs(ref[name])), (kind, n, name)


# ------------------------------------------------------------------------------------------------ surface
def test_module_surface_and_entry_point():
    import d3p_amd
    import d3p_amd._lib as L
    from d3p_amd import criteria as CR
    assert d3p_amd.loo is CR.loo and d3p_amd.posterior_loo is CR.posterior_loo and d3p_amd.LOOResult is CR.LOOResult
    assert all(name in d3p_amd.__all__ for name in ("loo", "posterior_loo", "LOOResult"))
    assert CR.LOOResult._fields == ("elpd_loo", "p_loo", "looic", "se", "n_draws", "n_rows", "k_threshold", "n_high_k", "pointwise")
    assert any(os.path.basename(p) == "d3p_psis.hip" for p in L._SRC) and all(p in L._DEPS for p in L._SRC)
    with open(os.path.join(ROOT, "include", "d3p_hip.h")) as f:
        hdr = f.read()
    assert re.search(r"\bint d3p_psis_loo\(", hdr) and re.search(r"#define D3P_ABI_VERSION 9\b", hdr)
    assert len(L.SIGNATURES["d3p_psis_loo"][1]) == 8
    lib = L.load()
    assert lib.d3p_abi_version() == 9 and hasattr(lib, "d3p_psis_loo")
    assert CR._k_threshold(1) == -math.inf and CR._k_threshold(100) == 0.5 and CR._k_threshold(10 ** 6) == 0.7
    assert CR._k_threshold(1000) == min(1.0 - 1.0 / math.log10(1000), 0.7)


def test_import_stays_lazy():
    code = "import sys, d3p_amd; assert 'torch' not in sys.modules and 'd3p_amd.criteria' not in sys.modules; " \
           "d3p_amd.loo; assert 'd3p_amd.criteria' in sys.modules"
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)


def test_slab_rows():
    from d3p_amd import infer_util as U
    assert U._loo_chunk(64, 64 << 20) == (64 << 20) // 256 and U._loo_chunk(64, 1) == 128 and U._loo_chunk(1000, 1 << 20) == 256
    assert U._loo_chunk(65535, 64 << 20) == 256 and U._loo_chunk(7, None) is None
    assert U._loo_chunk(3, 3 * 4 * 300) == 256 and U._loo_chunk(3, 3 * 4 * 384) == 384


# ------------------------------------------------------------------------------------------------ refusals
def test_loo_refuses_before_the_device(no_device):
    from d3p_amd import criteria as CR
    from d3p_amd.models import (AutoDiagonalNormal, GaussianMean, GaussianMixtureGuide, GaussianMixtureModel, LinearRegression,
                                LogisticRegression, PoissonRegression, VAEModel)
    X, y = np.zeros((6, 3), np.float32), np.zeros(6, np.float32)
    good = {"w": np.zeros((4, 3), np.float32)}
    key = torch.zeros(2, dtype=torch.int32)                                            # (a CPU tensor: the key check is the last)
    for bad_model in (GaussianMean(3), VAEModel(2, 4)):
        with pytest.raises(TypeError):
            CR.loo(bad_model, good, X, y)
        with pytest.raises(TypeError):
            CR.posterior_loo(key, 4, bad_model, (X, y), None, {})
    gm = GaussianMixtureModel()
    mix = {"pis": np.full((4, 3), 1 / 3, np.float32), "mus": np.zeros((4, 3, 2), np.float32), "sigs": np.ones((4, 3, 2), np.float32)}
    obs = np.zeros((10, 2), np.float32)
    big = np.broadcast_to(np.zeros((1, 3), np.float32), (65536, 3))
    for model in (LogisticRegression(3), LinearRegression(3), PoissonRegression(3)):
        for bad in (0, -5, 1.5, None, True, "64M"):
            with pytest.raises(ValueError, match="slab_bytes"):
                CR.loo(model, good, X, y, slab_bytes=bad)
        with pytest.raises(ValueError, match="65535"):
            CR.loo(model, {"w": big}, X, y)
        with pytest.raises(ValueError, match="y is missing"):
            CR.loo(model, good, X)
        with pytest.raises(ValueError):
            CR.loo(model, good)
        with pytest.raises(ValueError):
            CR.loo(model, {"intercept": np.zeros(4)}, X, y)
        guide = AutoDiagonalNormal(model)
        params = {"auto_loc": np.zeros(3, np.float32), "auto_scale": np.ones(3, np.float32)}
        with pytest.raises(ValueError, match="slab_bytes"):
            CR.posterior_loo(key, 4, model, (X, y), guide, params, slab_bytes=0)
        with pytest.raises(ValueError, match="65535"):
            CR.posterior_loo(key, 65536, model, (X, y), guide, params)
        with pytest.raises(ValueError, match="y is missing"):
            CR.posterior_loo(key, 4, model, (X,), guide, params)
        with pytest.raises(TypeError):
            CR.posterior_loo(key, 4, model, (X, y), guide, params)                     # every host check passed: the key is refused
    with pytest.raises(ValueError, match="slab_bytes"):
        CR.loo(gm, mix, obs, slab_bytes=0)
    with pytest.raises(ValueError, match="65535"):
        CR.loo(gm, {name: np.broadcast_to(v[:1], (65536,) + v.shape[1:]) for name, v in mix.items()}, obs)
    with pytest.raises(ValueError, match="obs is required"):
        CR.loo(gm, mix)
    with pytest.raises(ValueError):
        CR.loo(gm, {"pis": mix["pis"]}, obs)
    gg = GaussianMixtureGuide(gm)
    gparams = {"alpha_log": np.zeros(3, np.float32), "mus_loc": np.zeros((3, 2), np.float32)}
    with pytest.raises(ValueError, match="slab_bytes"):
        CR.posterior_loo(key, 4, gm, (3, obs, 10, 2), gg, gparams, slab_bytes=2.0)
    with pytest.raises(ValueError, match="65535"):
        CR.posterior_loo(key, 65536, gm, (3, obs, 10, 2), gg, gparams)
    with pytest.raises(ValueError, match="obs is required"):
        CR.posterior_loo(key, 4, gm, (3, None, 10, 2), gg, gparams)
    with pytest.raises(TypeError):
        CR.posterior_loo(key, 4, gm, (3, obs, 10, 2), gg, gparams)


# ------------------------------------------------------------------------------------------------ compare
def _hand_made(elpd, n=7):
    from d3p_amd import criteria as CR
    e = torch.tensor(np.asarray(elpd, np.float32))
    return CR._loo_result(e, e + 0.25, torch.full_like(e, 0.3), n, True)


def test_loo_result_of_hand_made_rows():
    from d3p_amd import criteria as CR
    e = torch.tensor([-1.0, -2.0, -4.0])
    k = torch.tensor([0.1, float("nan"), float("inf")])
    res = CR._loo_result(e, e + torch.tensor([0.5, 0.25, 1.0]), k, 100, True)
    assert float(res.elpd_loo) == -7.0 and float(res.p_loo) == 1.75 and float(res.looic) == 14.0 and res.k_threshold == 0.5
    assert res.n_high_k.dtype == torch.int64 and res.n_high_k.dim() == 0 and int(res.n_high_k) == 2
    assert all(t.dtype == torch.float64 and t.dim() == 0 for t in res[:4]) and (res.n_draws, res.n_rows) == (100, 3)
    assert sorted(res.pointwise) == ["elpd_loo", "lppd", "p_loo", "pareto_k"]
    assert abs(float(res.se) - math.sqrt(3 * np.var([-1.0, -2.0, -4.0], ddof=1))) <= 1e-14
    assert CR._loo_result(e, e, k, 100, False).pointwise is None


def test_compare_on_loo_results_and_mixed_kinds():
    from d3p_amd import criteria as CR
    r = np.random.default_rng(11)
    rows = 301
    ea = (-1.0 + 0.3 * r.normal(size=rows)).astype(np.float32)
    eb = (ea + 0.05 + 0.2 * r.normal(size=rows)).astype(np.float32)
    a, b = _hand_made(ea), _hand_made(eb, n=9)
    got = CR.compare(a, b)
    assert isinstance(got, CR.ComparisonResult) and got.elpd_diff.dtype == got.se_diff.dtype == torch.float64
    diff = ea.astype(np.float64) - eb.astype(np.float64)
    terms = rows * (diff - diff.mean()) ** 2 / (rows - 1)
    assert abs(float(got.elpd_diff) - diff.sum()) <= rows * 2.0 ** -52 * np.abs(diff).sum()
    assert abs(float(got.se_diff) ** 2 - terms.sum()) <= (rows + 2) * 2.0 ** -52 * terms.sum()
    assert float(CR.compare(b, a).elpd_diff) == -float(got.elpd_diff)
    pw = torch.zeros(rows)
    w = CR._result(torch.tensor(ea) + pw, pw, 7, True)
    for pair in ((a, w), (w, a)):
        with pytest.raises(ValueError, match="of a kind"):
            CR.compare(*pair)
    assert float(CR.compare(w, w).elpd_diff) == 0.0                                    # (WAIC results pair as before)
    with pytest.raises(ValueError, match="pointwise"):
        CR.compare(a, a._replace(pointwise=None))
    with pytest.raises(ValueError, match="rows"):
        CR.compare(a, _hand_made([-1.0, -2.0]))
