"""d3p_amd.mixture (predictive sampling and cluster assignment for the mixture model), host side: the key plan against a hand-written
split chain on oracle words, argument parsing and every refusal before a device is touched, the inverse mode map, and the
calibration of the assignment bound tests/test_gpu_mixture.py uses (tests/mixture_ref.py)."""
import os
import re

import numpy as np
import pytest
import torch

from . import mixture_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def no_device(monkeypatch):
    import d3p_amd._lib as L

    def refuse(*a, **k):
        raise AssertionError("mixture reached require_device")
    monkeypatch.setattr(L, "require_device", refuse)


def _mg():
    from d3p_amd.models import GaussianMixtureGuide, GaussianMixtureModel
    m = GaussianMixtureModel()
    return m, GaussianMixtureGuide(m)


def test_module_surface_and_entry_points():
    import d3p_amd
    import d3p_amd._lib as L
    from d3p_amd import mixture as MX
    assert d3p_amd.mixture is MX and "mixture" in d3p_amd.__all__
    assert MX.__all__ == ["prior_predictive_samples", "posterior_predictive_samples", "assignment_log_posterior", "assign",
                          "compute_assignment_accuracy", "ROW_TILE"]
    for name in MX.__all__[:5]:
        assert callable(getattr(MX, name))
    with open(os.path.join(ROOT, "include", "d3p_hip.h")) as f:
        hdr = f.read()
    for name in ("d3p_predict_gmm_draws", "d3p_predict_gmm_obs", "d3p_gmm_assign"):
        assert re.search(r"\bint " + name + r"\(", hdr) and name in L.SIGNATURES, name
    assert re.search(r"#define D3P_ABI_VERSION 9\b", hdr)
    with open(os.path.join(ROOT, "d3p_amd", "csrc", "d3p_predict_gmm.hip")) as f:
        src = f.read()
    tp = int(re.search(r"#define D3P_PGM_TP (\d+)", src).group(1))
    assert MX.ROW_TILE == 2 * tp and "#define D3P_PGM_ROW_TILE (2 * D3P_PGM_TP)" in src
    lib = L.load()
    assert lib.d3p_abi_version() == 9


def test_modelling_keeps_refusing_the_mixture_model():
    from d3p_amd import modelling as M
    m, _ = _mg()
    with pytest.raises(NotImplementedError):
        M.sample_prior_predictive(None, m, (3, None, 10, 2))


# ------------------------------------------------------------------------------------------------ key plan
def _split(O, key):
    kk = O.tf_split(key, 2)
    return kk[0], kk[1]


@pytest.mark.parametrize("subst", [(), ("pis",), ("mus",), ("sigs",), ("pis", "mus"), ("pis", "sigs"), ("mus", "sigs"),
                                   ("pis", "mus", "sigs")])
def test_prior_key_plan_against_a_hand_written_chain(O, subst):
    """The prior seeds the model's chain with the draw's key; every site that is not substituted takes `chain, key = split(chain)` in
    program order pis, mus, sigs, obs."""
    dk = R.key_words(77)
    got = R.site_keys(O, dk, False, subst)
    chain = dk
    for name in ("pis", "mus", "sigs", "obs"):
        if name in subst:
            assert got[name] is None
            continue
        chain, want = _split(O, chain)
        assert np.array_equal(got[name], want), name
    assert got["obs"] is not None


def test_posterior_key_plan_against_a_hand_written_chain(O):
    dk = R.key_words(78)
    got = R.site_keys(O, dk, True)
    model_key, guide_key = _split(O, dk)
    c, pis = _split(O, guide_key)
    c, mus = _split(O, c)
    c, sigs = _split(O, c)
    _, obs = _split(O, model_key)   # the three latents are substituted by the guide's draws: obs takes the model chain's key 0
    for name, want in (("pis", pis), ("mus", mus), ("sigs", sigs), ("obs", obs)):
        assert np.array_equal(got[name], want), name
    # the multi form: draw i runs on split(key, n)[i]; the single form on the key itself
    assert np.array_equal(R.draw_keys(O, dk, 3, True), O.tf_split(dk, 3)) and np.array_equal(R.draw_keys(O, dk, 1, False)[0], dk)


def test_key_plan_refusals():
    from d3p_amd import mixture as MX
    with pytest.raises(ValueError):
        MX._key_plan(False, ("obs",))
    with pytest.raises(ValueError):
        MX._key_plan(True, ("pis",))
    assert [s.key_index for s in MX._key_plan(False, ("mus",))] == [0, None, 1, 2]


# ------------------------------------------------------------------------------------------------ parsing and refusals
def test_shape_parsing_reads_the_arguments_as_the_reference_model():
    from d3p_amd import mixture as MX
    from d3p_amd.models import GaussianMixtureModel
    m = GaussianMixtureModel()
    assert MX._shape(m, (3, None, 10, 2), {}) == (3, 10, 2)
    assert MX._shape(m, (3, None), {"num_obs_total": 10, "d": 2}) == (3, 10, 2)
    assert MX._shape(m, (), {"k": 4, "num_obs_total": 7, "d": 5}) == (4, 7, 5)
    assert MX._shape(m, (3, np.zeros((6, 4))), {}) == (3, 6, 4)             # obs given: only its shape is used
    assert MX._shape(m, (3, np.zeros((6, 4)), 6, 9), {}) == (3, 6, 4)       # ... and d comes from it
    assert MX._shape(GaussianMixtureModel(k=5, d=3), (None, None, 8), {}) == (5, 8, 3)
    with pytest.raises(NotImplementedError):
        MX._shape(m, (3, np.zeros((6, 4)), 7), {})                           # plate mismatch, as modelling._check_plate
    for args, kw in (((3, None, None, 2), {}), ((3, None, 10), {}), ((None, None, 10, 2), {}), ((3, np.zeros(6)), {}), ((3, None, 0, 2), {})):
        with pytest.raises(ValueError):
            MX._shape(m, args, kw)


def test_every_refusal_comes_before_the_device(no_device):
    from d3p_amd import mixture as MX
    from d3p_amd.models import AutoDiagonalNormal, LogisticRegression
    m, g = _mg()
    key = torch.zeros(2, dtype=torch.int32)   # (a CPU tensor: not a threefry CUDA key)
    args = (3, None, 10, 2)
    params = {"alpha_log": np.zeros(3, np.float32), "mus_loc": np.zeros((3, 2), np.float32)}
    lr = LogisticRegression(2)
    with pytest.raises(TypeError):
        MX.prior_predictive_samples(key, 2, lr, args)
    with pytest.raises(TypeError):
        MX.posterior_predictive_samples(key, 2, lr, args, g, params)
    with pytest.raises(TypeError):
        MX.posterior_predictive_samples(key, 2, m, args, AutoDiagonalNormal(lr), params)
    with pytest.raises(TypeError):
        MX.posterior_predictive_samples(key, 2, m, args, None, params)
    with pytest.raises(ValueError):
        MX.prior_predictive_samples(key, 0, m, args)
    with pytest.raises(NotImplementedError):
        MX.prior_predictive_samples(key, 2, m, (3, np.zeros((10, 2)), 11))
    for bad in ({"obs": np.zeros((10, 2))}, {"pis": np.zeros(4)}, {"mus": np.zeros((2, 2))}, {"sigs": np.zeros((3, 3))}):
        with pytest.raises(ValueError):
            MX.prior_predictive_samples(key, 2, m, args, substitutes=bad)
    for bad in (None, {"alpha_log": np.zeros(3)}, {"alpha_log": np.zeros(4), "mus_loc": np.zeros((3, 2))},
                {"alpha_log": np.zeros(3), "mus_loc": np.zeros((2, 3))}):
        with pytest.raises(ValueError):
            MX.posterior_predictive_samples(key, 2, m, args, g, bad)
    for k, d in ((17, 256), (33, 1), (1, 257), (32, 129), (0, 2)):
        with pytest.raises(ValueError):
            MX.prior_predictive_samples(key, 2, m, (k, None, 10, d))
    with pytest.raises(ValueError):
        MX.prior_predictive_samples(key, 2, m, (1, None, 2 ** 32, 1))
    with pytest.raises(ValueError):
        MX.prior_predictive_samples(key, 2, m, (2, None, 2 ** 24, 256))
    for bad_key in (key, None, torch.zeros(3, dtype=torch.int32), np.zeros(2, np.uint32)):   # the key's type is the last host check
        with pytest.raises(TypeError):
            MX.prior_predictive_samples(bad_key, 2, m, args, substitutes={"sigs": np.ones((3, 1))})
        with pytest.raises(TypeError):
            MX.posterior_predictive_samples(bad_key, None, m, args, g, params)
    obs, mus, sigs, pis = R.assign_inputs(3, 2, 4)
    for fn in (MX.assignment_log_posterior, MX.assign):
        for bad in ((obs[0], mus, sigs, pis), (obs, mus[:, :1], sigs, pis), (obs, mus, sigs[:2], pis), (obs, mus, sigs, pis[:2]),
                    (np.zeros((2, 257), np.float32), np.zeros((1, 257), np.float32), np.ones((1, 257), np.float32), np.ones(1, np.float32))):
            with pytest.raises(ValueError):
                fn(*bad)


# ------------------------------------------------------------------------------------------------ the inverse mode map
def test_inverse_mode_map_on_a_non_bijective_case():
    """Reference :142-146: the identity as a base, then inv[mode_map[j]] = j in order of j."""
    from d3p_amd import mixture as MX
    assert MX.inverse_mode_map([2, 0, 1], 3) == {2: 0, 0: 1, 1: 2}
    # true modes 0 and 1 both claim learned component 2: it stands for the later one; the unclaimed component 1 for itself
    assert MX.inverse_mode_map([2, 2, 0], 3) == {0: 2, 1: 1, 2: 1}
    assert MX.inverse_mode_map([1, 1, 1], 3) == {0: 0, 1: 2, 2: 2}


# ------------------------------------------------------------------------------------------------ the comparator's own checks
def test_component_rule_edges():
    assert list(R.component_rule([1, 0, 0], [0.0, 0.5, 0.99999994])) == [0, 0, 0]
    assert list(R.component_rule([0, 0, 1], [1e-9, 0.5])) == [2, 2]
    tenth = np.full(10, 0.1, np.float32)
    top = np.cumsum(tenth, dtype=np.float32)[-1]
    # a uniform above the last running sum counts all k components and is clamped to k - 1
    assert list(R.component_rule(tenth, [np.nextafter(top, np.float32(2))])) == [9] and list(R.component_rule(tenth, [top])) == [9]
    assert list(R.component_rule(tenth, [np.float32(0.05), np.float32(0.15)])) == [0, 1]


def test_assignment_bound_calibration():
    """The numpy float32 restatement of the direct form against the float64 comparator over the GPU tests' inputs: the largest
    error in units of 2^-24 x the condition scale is what tests/mixture_ref.py records, and the bound is four times that."""
    worst = 0.0
    for k, d, rows in R.SHAPES:
        obs, mus, sigs, pis = R.assign_inputs(k, d, rows)
        a, scale = R.a64(obs, mus, sigs, pis)
        err = np.abs(R.a32_restated(obs, mus, sigs, pis).astype(np.float64) - a) / (2.0 ** -24 * scale)
        print(f"k={k} d={d} rows={rows}: max scaled error {err.max():.3f} ulps")
        worst = max(worst, float(err.max()))
    print(f"largest: {worst:.3f}")
    assert worst <= R.A_ERR_SEEN_ULPS and worst >= 0.9 * R.A_ERR_SEEN_ULPS, worst   # (the record is what the run gives)
    assert R.A_BOUND_ULPS == pytest.approx(4 * R.A_ERR_SEEN_ULPS, rel=0.01)


def test_comparator_alone_leaves_nothing_unjudged_on_the_toy_clusters():
    """Three clusters at -10, 10, -2 with scales 0.1, 1, 0.1: the float64 top-two gap exceeds twice the bound in every row, and the
    float32 restatement assigns as the comparator does."""
    for k, d, rows in R.SHAPES:
        obs, mus, sigs, pis = R.assign_inputs(k, d, rows)
        a, scale = R.a64(obs, mus, sigs, pis)
        judged = R.judged_rows(a, R.a_bound(scale))
        if k <= 3:
            assert judged.all(), (k, d, rows)
        R.assert_not_vacuous(1.0 - judged.mean(), rows, f"k={k} d={d} rows={rows}")
        a32 = R.a32_restated(obs, mus, sigs, pis)
        assert np.array_equal(a32.argmax(axis=1)[judged], a.argmax(axis=1)[judged])
        assert np.all(np.abs(a32 - a) <= R.a_bound(scale))


# ------------------------------------------------------------------------------------------------ the outcome kernel's tile plan
@pytest.mark.parametrize("rows,d", [(1, 1), (2, 1), (3, 5), (R.T - 1, 2), (R.T, 2), (R.T + 1, 2), (5, 256), (5, 128), (2 * R.T + 1, 5),
                                    (300, 64), (1000, 1), (257, 3), (131, 255), (513, 2)])
def test_outcome_tile_plan_covers_every_element_once(rows, d):
    """The pair tile of k_predict_gmm_obs restated in Python (tests/mixture_ref.py: obs_tile_plan): every outcome and every zs row is
    written exactly once, every pair's (row, column) is the element's, and the staged component arrays are read inside their
    D3P_PGM_TP and D3P_PGM_TP + 1 rows."""
    with open(os.path.join(ROOT, "d3p_amd", "csrc", "d3p_predict_gmm.hip")) as f:
        tp = int(re.search(r"#define D3P_PGM_TP (\d+)", f.read()).group(1))
    wrote, zs, top = R.obs_tile_plan(rows, d, tp)
    assert np.all(wrote == 1) and np.all(zs == 1)
    assert top[0] <= tp - 1 and top[1] <= tp


def test_example_parser_has_the_two_opt_in_flags():
    import importlib.util
    spec = importlib.util.spec_from_file_location("ex_gmm_args", os.path.join(ROOT, "examples", "gaussian_mixture_model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    a = mod.parse_args([])
    assert (a.toy_data, a.assignment) == ("torch", "modes")                      # the defaults stay as they were
    a = mod.parse_args("--toy-data predictive --assignment posterior --sigma 1.0 -N 512 -n 2".split())
    assert (a.toy_data, a.assignment, a.sigma, a.num_samples, a.num_epochs) == ("predictive", "posterior", 1.0, 512, 2)
    with pytest.raises(SystemExit):
        mod.parse_args(["--toy-data", "other"])
