"""d3p_amd.ppc (posterior predictive checks), host side: the module and its C entries exist, every refusal is raised before a device is
touched, the p-value and ReplicateStats arithmetic is right on hand-made numbers -- and the self-checks of tests/ppc_ref.py, the
restatement every comparison of tests/test_gpu_ppc.py rests on."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from . import ppc_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def no_device(monkeypatch):
    import d3p_amd._lib as L

    def refuse(*a, **k):
        raise AssertionError("ppc reached require_device")
    monkeypatch.setattr(L, "require_device", refuse)


def test_header_and_binding_declare_the_three_symbols():
    import d3p_amd._lib as L
    with open(os.path.join(ROOT, "include", "d3p_hip.h")) as f:
        hdr = f.read()
    assert re.search(r"#define D3P_ABI_VERSION 9\b", hdr)
    assert re.search(r"\bsize_t d3p_rep_stats_workspace\(uint64_t rows, uint32_t n\);", hdr)
    assert re.search(r"\bint d3p_rep_stats\(void\* stream, const void\* m_dev, int32_t dtype, int64_t ld, uint32_t n, uint64_t rows, double shift,", hdr)
    assert re.search(r"\bint d3p_predict_stats\(void\* stream, const d3p_logreg_model\* model, const float\* X_dev, uint64_t rows, int32_t d,", hdr)
    arity = {"d3p_rep_stats_workspace": 2, "d3p_rep_stats": 10, "d3p_predict_stats": 15}
    for name, n in arity.items():
        args = re.search(r"\b" + name + r"\(([^)]*)\);", hdr).group(1)
        assert args.count(",") + 1 == n == len(L.SIGNATURES[name][1]), name
    assert L.SIGNATURES["d3p_rep_stats_workspace"][0] is L.C.c_size_t and L.SIGNATURES["d3p_rep_stats"][0] is L.C.c_int
    assert L.SIGNATURES["d3p_rep_stats"][1][6] is L.C.c_double and L.SIGNATURES["d3p_predict_stats"][1][11] is L.C.c_double
    csrc = os.path.join(os.path.dirname(L.__file__), "csrc")
    assert os.path.join(csrc, "d3p_rep_stats.hip") in L._SRC and os.path.join(csrc, "d3p_outcome.h") in L._DEPS
    lib = L.load()
    assert lib.d3p_abi_version() == 9
    for name in arity:
        assert getattr(lib, name).argtypes == L.SIGNATURES[name][1]


def test_workspace_size_follows_the_strip_function():
    import d3p_amd._lib as L
    lib = L.load()
    for rows, n in ((1, 1), (128, 7), (129, 128), (65536, 3), (65537, 3), (10 ** 6, 128)):
        assert lib.d3p_rep_stats_workspace(rows, n) == R.strips(rows)[2] * 5 * n * 8
    assert lib.d3p_rep_stats_workspace(0, 4) == 0 and lib.d3p_rep_stats_workspace(2 ** 32, 4) == 0


def test_strip_function():
    assert R.strips(128) == (1, 1, 1)
    assert R.strips(65537) == (513, 2, 257)
    assert R.strips(65536) == (512, 1, 512)
    assert R.strips(1) == (1, 1, 1) and R.strips(129) == (2, 1, 2) and R.strips(10 ** 6) == (7813, 16, 489)


def test_c_refusals_that_need_no_device():
    """Argument errors of d3p_rep_stats that are decided before any pointer is examined on a device."""
    import d3p_amd._lib as L
    lib = L.load()
    buf = np.zeros(64, np.float64)
    p = buf.ctypes.data
    assert lib.d3p_rep_stats(None, None, 0, 4, 1, 4, 0.0, p, p, 64) == -1 and b"null" in lib.d3p_last_error()
    assert lib.d3p_rep_stats(None, p + 2, 0, 4, 1, 4, 0.0, p, p, 64) == -1 and b"aligned" in lib.d3p_last_error()
    assert lib.d3p_rep_stats(None, p, 0, 4, 1, 4, 0.0, p + 4, p, 64) == -1 and b"aligned" in lib.d3p_last_error()
    assert lib.d3p_rep_stats(None, p, 2, 4, 1, 4, 0.0, p, p, 64) == -1 and b"dtype" in lib.d3p_last_error()
    assert lib.d3p_rep_stats(None, p, 0, 4, 0, 4, 0.0, p, p, 64) == -1 and b"n must be" in lib.d3p_last_error()
    assert lib.d3p_rep_stats(None, p, 0, 4, 1, 0, 0.0, p, p, 64) == -1 and b"rows must be" in lib.d3p_last_error()
    assert lib.d3p_rep_stats(None, p, 0, 3, 1, 4, 0.0, p, p, 64) == -1 and b"ld >= rows" in lib.d3p_last_error()
    assert lib.d3p_rep_stats(None, p, 1, 4, 1, 4, math.inf, p, p, 64) == -1 and b"finite" in lib.d3p_last_error()
    assert lib.d3p_rep_stats(None, p, 1, 4, 1, 4, math.nan, p, p, 64) == -1 and b"finite" in lib.d3p_last_error()
    assert lib.d3p_rep_stats(None, p, 0, 2 ** 32, 1, 2 ** 32, 0.0, p, p, 64) == -3
    assert lib.d3p_rep_stats(None, p, 0, 4, 128 * 65535 + 1, 4, 0.0, p, p, 64) == -3
    assert lib.d3p_rep_stats(None, p, 0, 4, 1, 4, 0.0, p, p, 39) == -1 and b"40 needed" in lib.d3p_last_error()
    assert lib.d3p_rep_stats(None, p, 0, 4, 1, 4, 0.0, p, None, 64) == -1 and b"workspace" in lib.d3p_last_error()


def test_module_surface_and_lazy_import():
    import d3p_amd
    from d3p_amd import ppc
    assert d3p_amd.ppc is ppc and "ppc" in d3p_amd.__all__
    assert ppc.__all__ == ["replicate_stats", "predictive_stats", "posterior_predictive_stats", "posterior_predictive_check", "ReplicateStats",
                           "PPCResult", "STATISTICS"]
    assert ppc.ReplicateStats._fields == ("sum", "sumsq", "min", "max", "zeros", "n_rows", "shift")
    assert ppc.PPCResult._fields == ("statistic", "observed", "replicated", "p_ge", "p_le", "n_draws", "n_rows", "n_marked")
    code = "import sys, d3p_amd; assert 'torch' not in sys.modules and 'd3p_amd.ppc' not in sys.modules; " \
           "d3p_amd.ppc; assert 'd3p_amd.ppc' in sys.modules"
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)


def test_each_outcome_rule_is_defined_once():
    csrc = os.path.join(ROOT, "d3p_amd", "csrc")
    counts = {r"int32_t poisson_draw\(": 0, r"int32_t bernoulli_draw\(": 0, r"float sigmoid_probs\(": 0, r"void glm_uniform_pair\(": 0,
              r"float normal_site_value\(": 0}
    for name in os.listdir(csrc):
        with open(os.path.join(csrc, name)) as f:
            text = f.read()
        for pat in counts:
            counts[pat] += len(re.findall(pat, text))
    assert all(c == 1 for c in counts.values()), counts
    with open(os.path.join(csrc, "d3p_rep_stats.hip")) as f:
        text = f.read()
    with open(os.path.join(csrc, "d3p_outcome.h")) as f:
        outcome = f.read()
    choice = outcome[outcome.index("auto glm_outcome("):]   # the one choice among the rules, built on the one definition of each
    for call in ("poisson_draw(", "bernoulli_draw(", "sigmoid_probs(", "normal_site_value(", "tile_product(", "tile_scatter("):
        assert call in text or ("glm_outcome<FAMILY>(" in text and call in choice), call   # the fused kernel applies the shared rules, not copies
    assert "atomic" not in text.lower().replace("no floating-point atomics", "")


def test_replicate_stats_refusals(no_device):
    from d3p_amd import ppc
    with pytest.raises(TypeError, match="CUDA tensor"):
        ppc.replicate_stats(np.zeros((2, 3), np.float32))
    with pytest.raises(TypeError, match="float32 or int32"):
        ppc.replicate_stats(torch.zeros(2, 3, dtype=torch.float64))
    with pytest.raises(TypeError, match="float32 or int32"):
        ppc.replicate_stats(torch.zeros(2, 3, dtype=torch.int64))
    with pytest.raises(ValueError, match="shape"):
        ppc.replicate_stats(torch.zeros(2, 3, 4))
    with pytest.raises(ValueError, match="at least one"):
        ppc.replicate_stats(torch.zeros(2, 0))
    with pytest.raises(ValueError, match="at least one"):
        ppc.replicate_stats(torch.zeros(0, dtype=torch.int32))
    for bad in (math.inf, -math.inf, math.nan):
        with pytest.raises(ValueError, match="finite"):
            ppc.replicate_stats(torch.zeros(2, 3), shift=bad)
    with pytest.raises(TypeError, match="CUDA tensor"):          # what passes every check arrives at the device check
        ppc.replicate_stats(torch.zeros(2, 3))


def test_sampling_refusals_are_kept(no_device):
    from d3p_amd import ppc
    from d3p_amd.models import (AutoDiagonalNormal, DiagonalNormalGuide, GaussianMean, GaussianMixtureModel, LinearRegression,
                                LogisticRegression, MeanFieldGuide, PoissonRegression, VAEGuide, VAEModel)
    X, y = torch.zeros(5, 3), torch.zeros(5)
    lin, poi, logi = LinearRegression(3, intercept=True), PoissonRegression(3, intercept=True), LogisticRegression(3, intercept=True)
    auto = {"auto_loc": torch.zeros(4), "auto_scale": torch.ones(4)}
    w = {"w": torch.zeros(4, 3), "intercept": torch.zeros(4)}
    post = (lambda n, model, args, guide, params, **k: ppc.posterior_predictive_stats(None, n, model, args, guide, params, **k),
            lambda n, model, args, guide, params, **k: ppc.posterior_predictive_check(None, n, model, args, guide, params, **k))
    for bad in (GaussianMean(3), GaussianMixtureModel(2, 3), VAEModel(2, 3)):
        with pytest.raises(TypeError, match="unsupported model"):
            ppc.predictive_stats(None, bad, w, X)
        for f in post:
            with pytest.raises(TypeError, match="unsupported model"):
                f(4, bad, (X, y), AutoDiagonalNormal(lin), auto)
    for f in post:
        for model in (lin, poi):
            with pytest.raises(TypeError, match="MeanFieldGuide is not supported"):
                f(4, model, (X, y), MeanFieldGuide(model), {})
        with pytest.raises(TypeError, match="VAEGuide is not supported"):
            f(4, logi, (X, y), VAEGuide(VAEModel(2, 3)), {})
        for n in (0, -2):
            with pytest.raises(ValueError, match="n must be >= 1"):
                f(n, lin, (X, y), AutoDiagonalNormal(lin), auto)
        with pytest.raises(ValueError, match="model_args"):
            f(4, lin, (), AutoDiagonalNormal(lin), auto)
        with pytest.raises(ValueError, match="columns"):
            f(4, LinearRegression(4, intercept=True), (X, y), AutoDiagonalNormal(lin), auto)
        with pytest.raises(NotImplementedError, match="num_obs_total = 7"):
            f(4, lin, (X, y, 7), AutoDiagonalNormal(lin), auto)
        with pytest.raises(ValueError, match="params"):
            f(4, lin, (X, y), AutoDiagonalNormal(lin), None)
        with pytest.raises(ValueError, match="'auto_scale' is missing"):
            f(4, lin, (X, y), AutoDiagonalNormal(lin), {"auto_loc": torch.zeros(4)})
        with pytest.raises(ValueError, match="'w_std_log' is missing"):
            f(4, poi, (X, y), DiagonalNormalGuide(poi), {"w_loc": torch.zeros(4)})
        with pytest.raises(TypeError, match="rng_key"):             # everything passes: the key is the last check before the device
            f(4, poi, (X, y), AutoDiagonalNormal(poi), auto)
        with pytest.raises(TypeError, match="rng_key"):
            f(4, logi, (X, y), MeanFieldGuide(logi), {"w_loc": torch.zeros(3), "w_std_log": torch.zeros(3), "intercept_loc": torch.zeros(1),
                                                      "intercept_std_log": torch.zeros(1)})
    with pytest.raises(ValueError, match="finite"):
        ppc.posterior_predictive_stats(None, 4, lin, (X,), AutoDiagonalNormal(lin), auto, shift=math.nan)
    # predictive_stats: predictive_samples' checks
    with pytest.raises(ValueError, match="'w' is missing"):
        ppc.predictive_stats(None, lin, {}, X)
    with pytest.raises(ValueError, match="'intercept' is missing"):
        ppc.predictive_stats(None, lin, {"w": torch.zeros(4, 3)}, X)
    with pytest.raises(ValueError, match="2-D"):
        ppc.predictive_stats(None, lin, w, torch.zeros(5))
    with pytest.raises(NotImplementedError, match="num_obs_total = 9"):
        ppc.predictive_stats(None, lin, w, X, y, 9)
    with pytest.raises(ValueError, match="finite"):
        ppc.predictive_stats(None, lin, w, X, shift=math.inf)
    with pytest.raises(TypeError, match="rng_key"):
        ppc.predictive_stats(None, lin, w, X, y, shift=1.5)


def test_check_refusals(no_device):
    from d3p_amd import ppc
    from d3p_amd.models import AutoDiagonalNormal, LinearRegression, LogisticRegression, PoissonRegression
    X = torch.zeros(5, 3)
    poi, logi, lin = PoissonRegression(3), LogisticRegression(3), LinearRegression(3)
    auto = {"auto_loc": torch.zeros(3), "auto_scale": torch.ones(3)}
    f = ppc.posterior_predictive_check
    with pytest.raises(ValueError, match="unknown statistic 'median'"):
        f(None, 4, poi, (X, torch.zeros(5)), AutoDiagonalNormal(poi), auto, statistics=("mean", "median"))
    with pytest.raises(ValueError, match="at least one"):
        f(None, 4, poi, (X, torch.zeros(5)), AutoDiagonalNormal(poi), auto, statistics=())
    with pytest.raises(ValueError, match="y is missing"):
        f(None, 4, poi, (X,), AutoDiagonalNormal(poi), auto)
    with pytest.raises(ValueError, match="5 values expected"):
        f(None, 4, poi, (X, torch.zeros(4)), AutoDiagonalNormal(poi), auto)
    for model in (poi, logi):
        with pytest.raises(ValueError, match="non-integral"):
            f(None, 4, model, (X, torch.tensor([0.0, 1.0, 0.5, 1.0, 0.0])), AutoDiagonalNormal(model), auto)
        with pytest.raises(ValueError, match="non-integral"):
            f(None, 4, model, (X, np.array([0.0, 1.0, np.nan, 1.0, 0.0])), AutoDiagonalNormal(model), auto)
        with pytest.raises(TypeError, match="rng_key"):             # integral floats pass
            f(None, 4, model, (X, torch.tensor([0.0, 1.0, 1.0, 1.0, 0.0])), AutoDiagonalNormal(model), auto, statistics="zeros")
    with pytest.raises(TypeError, match="rng_key"):                 # any float is an outcome of the linear family
        f(None, 4, lin, (X, torch.tensor([0.0, 1.0, 0.5, 1.0, 0.0])), AutoDiagonalNormal(lin), auto)


def test_tail_shares_by_value_with_ties():
    from d3p_amd import ppc
    rep = np.array([1.0, 2.0, 2.0, 3.0, 5.0])
    assert ppc._tail_shares(rep, 2.0) == (0.8, 0.6)              # ties count on both sides
    assert ppc._tail_shares(rep, 0.0) == (1.0, 0.0)
    assert ppc._tail_shares(rep, 6.0) == (0.0, 1.0)
    assert ppc._tail_shares(rep, 2.5) == (0.4, 0.6)
    assert ppc._tail_shares(np.array([0.0, -0.0]), 0.0) == (1.0, 1.0)        # by value: -0 equals +0
    assert ppc._tail_shares(np.array([np.nan, 1.0]), 1.0) == (0.5, 0.5)      # a NaN counts on neither side
    assert ppc._tail_shares(np.array([1.0, 2.0]), np.nan) == (0.0, 0.0)


def test_replicate_stats_properties_on_hand_made_numbers():
    from d3p_amd import ppc
    # two data sets of 4 rows with shift 2: {1, 2, 3, 6} and {0, 0, 0, 4}
    v = np.array([[1.0, 2.0, 3.0, 6.0], [0.0, 0.0, 0.0, 4.0]])
    e = v - 2.0
    t = lambda a: torch.tensor(a, dtype=torch.float64)
    rs = ppc.ReplicateStats(t(e.sum(1)), t((e * e).sum(1)), t(v.min(1)), t(v.max(1)), t((v == 0).sum(1).astype(float)), 4, 2.0)
    assert rs.mean.tolist() == [3.0, 1.0]
    assert rs.var().tolist() == [14.0 / 3.0, 4.0] and rs.var(ddof=0).tolist() == [3.5, 3.0]
    assert rs.sd.tolist() == [math.sqrt(14.0 / 3.0), 2.0]
    assert rs.zero_share.tolist() == [0.0, 0.75]
    assert rs.dispersion.tolist() == [(14.0 / 3.0) / 3.0, 4.0]
    assert rs.mean.dtype == torch.float64 and rs.dispersion.dtype == torch.float64
    for name, want in (("mean", rs.mean), ("var", rs.var()), ("sd", rs.sd), ("zero_share", rs.zero_share), ("dispersion", rs.dispersion),
                       ("min", rs.min), ("max", rs.max), ("zeros", rs.zeros)):
        assert torch.equal(ppc._derive(name, rs._five(), 4, 2.0), want), name      # the names posterior_predictive_check takes
    assert sorted(ppc.STATISTICS) == sorted(["mean", "var", "sd", "zero_share", "dispersion", "min", "max", "zeros"])
    with pytest.raises(ValueError, match="unknown statistic"):
        ppc._derive("median", rs._five(), 4, 2.0)
    # the same arithmetic on numpy arrays (what posterior_predictive_check runs on the host)
    five = [np.asarray(x) for x in rs._five()]
    assert ppc._derive("sd", five, 4, 2.0).tolist() == rs.sd.tolist() and ppc._derive("mean", five, 4, 2.0).tolist() == [3.0, 1.0]
    one = ppc.ReplicateStats(t([0.0]), t([0.0]), t([2.0]), t([2.0]), t([0.0]), 1, 2.0)
    assert math.isnan(float(one.var()[0])) and float(one.var(ddof=0)[0]) == 0.0 and float(one.mean[0]) == 2.0


def test_ppc_result_lines():
    from d3p_amd import ppc
    rep = {"mean": np.array([1.0, 2.0, 3.0]), "zeros": np.array([np.nan, np.nan, np.nan])}
    res = ppc.PPCResult(("mean", "zeros"), {"mean": 2.0, "zeros": 7.0}, rep, {"mean": 2 / 3, "zeros": 0.0}, {"mean": 2 / 3, "zeros": 0.0}, 3, 10, 0)
    lines = res.lines()
    assert len(lines) == 2 and lines[0].startswith("ppc mean") and "p_ge 0.667" in lines[0] and "nan" in lines[1]


@pytest.mark.parametrize("rows", [1, 33, 129, 300, 1000])
def test_restatement_against_fsum_and_exact_integers(rows):
    rng = np.random.default_rng(rows)
    n = 3
    mf = (rng.normal(size=(n, rows)) * 10 ** rng.uniform(-2, 3, size=(n, 1))).astype(np.float32)
    for shift in (0.0, 1.25, float(np.float32(mf.mean()))):
        got, ref = R.rep_stats(mf, shift), R.rep_stats_naive(mf, shift)
        e = np.abs(mf.astype(np.float64) - shift)
        assert np.all(np.abs(got[0] - ref[0]) <= rows * 2.0 ** -53 * e.sum(1))
        assert np.all(np.abs(got[1] - ref[1]) <= rows * 2.0 ** -53 * (e * e).sum(1))      # (the same rounded products on both sides)
        assert np.array_equal(got[2:], ref[2:])
    mi = rng.integers(-1000, 1000, size=(n, rows)).astype(np.int32)
    mi[0, 0] = 0
    for shift in (0.0, 3.0, -17.0):                                   # integral shifts: every term and every partial sum is an integer
        got = R.rep_stats(mi, shift)
        e = mi.astype(np.int64) - int(shift)
        assert np.array_equal(got[0], e.sum(1)) and np.array_equal(got[1], (e * e).sum(1))
        assert np.array_equal(got[2], mi.min(1)) and np.array_equal(got[3], mi.max(1)) and np.array_equal(got[4], (mi == 0).sum(1))
        assert np.array_equal(got, R.rep_stats_naive(mi, shift))


def test_restatement_special_values():
    m = np.array([[0.0, -0.0, 1.0, np.inf], [np.nan, 0.0, 2.0, 3.0], [-np.inf, 5.0, 5.0, np.inf], [7.0, 7.0, 7.0, 7.0]], np.float32)
    s = R.rep_stats(m, 0.5)
    assert s[4].tolist() == [2.0, 1.0, 0.0, 0.0]                        # -0.0 counts, NaN does not
    assert np.isnan(s[:4, 1]).all() and s[4, 1] == 1.0                   # a NaN: outputs 0..3 of that draw, and no other draw
    assert s[0, 0] == np.inf and s[3, 0] == np.inf and s[2, 0] == 0.0
    assert np.isnan(s[0, 2]) and s[1, 2] == np.inf and s[2, 2] == -np.inf and s[3, 2] == np.inf   # inf - inf in the sum only
    assert s[:, 3].tolist() == [26.0, 169.0, 7.0, 7.0, 0.0]
    assert R.same(s[:, 0], R.rep_stats(m[0], 0.5)[:, 0])                 # a draw does not depend on the others
    lim = np.array([[-2 ** 31, 2 ** 31 - 1, 0, -1]], np.int32)
    s = R.rep_stats(lim, 0.0)
    assert s[:, 0].tolist() == [-2.0, 2.0 ** 62 + (2.0 ** 31 - 1) ** 2 + 1.0, -2.0 ** 31, 2.0 ** 31 - 1, 1.0]


def test_poisson_check_margin_on_the_cpu():
    """Check (b) of tests/test_gpu_ppc.py, restated with tests/predictive_glm_ref.py's Poisson rule on grid uniforms: 2000 rows at a
    predictor near 2 (rate e^2 = 7.4), half of y set to 0.  A replicated data set holds about 2000 e^-7.4 = 1.2 zeros against >= 1000
    observed, and its dispersion stays near 1 against an observed one above 4 -- for any key, so no seed is special."""
    from . import predictive_glm_ref as G
    rows, n = 2000, 64
    rng = np.random.default_rng(11)
    t = 2.0 + 1e-3 * rng.normal(size=(n, rows))
    lam = np.exp(t.astype(np.float32)).astype(np.float64)
    k = G.poisson_rule(lam[None], G.GridUniforms(rng, (n, rows)))[0][0].astype(np.int32)
    rep = R.rep_stats(k, 0.0)
    assert rep[4].max() <= 12                                        # P(Poisson(1.2) > 12) < 1e-9
    y = k[0].copy()
    y[::2] = 0
    obs = R.rep_stats(y, 0.0)[:, 0]
    assert obs[4] >= 1000
    disp = lambda s: ((s[1] - s[0] ** 2 / rows) / (rows - 1)) / (s[0] / rows)
    assert disp(rep).max() < 1.3 and disp(obs) > 3.0
