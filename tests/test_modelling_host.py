"""Predictive sampling (d3p_amd.modelling) without a GPU: the per-family site plan as a property, and the argument checks that
must fire before any device call."""
import itertools

import numpy as np
import pytest
import torch

from d3p_amd import modelling as M
from d3p_amd.models import (AutoDiagonalNormal, DiagonalNormalGuide, GaussianMean, GaussianMixtureGuide, GaussianMixtureModel,
                            LogisticRegression, MeanFieldGuide, VAEGuide, VAEModel)


def _families():
    lr, lri, gm, vae = LogisticRegression(3), LogisticRegression(3, intercept=True), GaussianMean(2), VAEModel(4, 8)
    dims = dict(d=3, rows=7, B=2, Z=4, D=6)
    return [(lr, None), (lri, None), (gm, None), (vae, None), (lr, AutoDiagonalNormal(lr)), (lri, AutoDiagonalNormal(lri)),
            (lri, MeanFieldGuide(lri)), (lr, DiagonalNormalGuide(lr)), (gm, DiagonalNormalGuide(gm)), (gm, AutoDiagonalNormal(gm)),
            (vae, VAEGuide(vae))], dims


def test_site_plan_orders_and_keys():
    lri = LogisticRegression(3, intercept=True)
    plan = M.site_plan(lri, None, d=3, rows=5)
    assert [(s.name, s.size, s.chain, s.key_index) for s in plan] == [("w", 3, "model", 0), ("intercept", 1, "model", 1), ("obs", 5, "model", 2)]
    plan = M.site_plan(lri, MeanFieldGuide(lri), d=3, rows=5)
    assert [(s.name, s.chain, s.key_index, s.substituted) for s in plan] == [
        ("w", "guide", 0, False), ("intercept", "guide", 1, False), ("w", "model", None, True), ("intercept", "model", None, True),
        ("obs", "model", 0, False)]
    plan = M.site_plan(lri, AutoDiagonalNormal(lri), d=3, rows=5)
    assert [(s.name, s.size, s.chain, s.key_index) for s in plan if not s.substituted] == [("_auto_latent", 4, "guide", 0), ("obs", 5, "model", 0)]
    plan = M.site_plan(VAEModel(4, 8), None, d=None, rows=None, B=2, Z=4, D=6)
    assert [(s.name, s.size, s.key_index) for s in plan] == [("z", 8, 0), ("obs", 12, 1)]


@pytest.mark.parametrize("case", range(11))
def test_substituting_a_site_removes_exactly_its_key(case):
    """Property: substituting one site drops its key and moves every later key of the same handler one index down; nothing else moves."""
    fams, dims = _families()
    model, guide = fams[case]
    base = M.site_plan(model, guide, **dims)
    names = [s.name for s in base if s.chain == "model" and not s.substituted]
    for r in range(1, len(names) + 1):
        for subset in itertools.combinations(names, r):
            plan = M.site_plan(model, guide, set(subset), **dims)
            assert [(s.name, s.size, s.chain) for s in plan] == [(s.name, s.size, s.chain) for s in base]
            for b, p in zip(base, plan):
                if b.chain != "model" or b.substituted:
                    assert p == b
                elif b.name in subset:
                    assert p.substituted and p.key_index is None
                else:
                    removed_before = sum(1 for q in base[:base.index(b)] if q.chain == "model" and q.name in subset)
                    assert p.key_index == b.key_index - removed_before and not p.substituted
            # the key indices left under each handler are 0 .. k-1 in program order
            for ch in ("model", "guide"):
                ks = [p.key_index for p in plan if p.chain == ch and p.key_index is not None]
                assert ks == list(range(len(ks)))


def _no_cuda_key():
    return torch.zeros(2, dtype=torch.int32)


def test_gmm_raises_not_implemented():
    gmm = GaussianMixtureModel(3, 2)
    with pytest.raises(NotImplementedError, match="follow-up"):
        M.sample_prior_predictive(_no_cuda_key(), gmm, (3, None), num_obs_total=10)
    with pytest.raises(NotImplementedError):
        M.sample_multi_posterior_predictive(_no_cuda_key(), 4, gmm, (3, None), GaussianMixtureGuide(gmm), (3, None), {})


def test_num_obs_total_other_than_rows_raises_not_implemented():
    X = np.zeros((10, 3), np.float32)
    lr = LogisticRegression(3)
    with pytest.raises(NotImplementedError, match="subsample"):
        M.sample_prior_predictive(_no_cuda_key(), lr, (X,), num_obs_total=20)
    with pytest.raises(NotImplementedError):
        M.sample_prior_predictive(_no_cuda_key(), lr, (X, None, 11))
    with pytest.raises(NotImplementedError):
        M.sample_prior_predictive(_no_cuda_key(), GaussianMean(2), (np.zeros((5, 2), np.float32), 6))
    with pytest.raises(NotImplementedError):
        M.sample_prior_predictive(_no_cuda_key(), VAEModel(4, 8), (3, 4, 8, 6), num_obs_total=4)


def test_missing_or_mis_sized_params_raise_value_error():
    X = np.zeros((10, 3), np.float32)
    lri = LogisticRegression(3, intercept=True)
    key = _no_cuda_key()
    with pytest.raises(ValueError, match="auto_scale"):
        M.sample_posterior_predictive(key, lri, (X,), AutoDiagonalNormal(lri), (X,), {"auto_loc": np.zeros(4)})
    with pytest.raises(ValueError, match="4 values"):
        M.sample_posterior_predictive(key, lri, (X,), AutoDiagonalNormal(lri), (X,), {"auto_loc": np.zeros(3), "auto_scale": np.ones(4)})
    with pytest.raises(ValueError):
        M.sample_multi_posterior_predictive(key, 3, lri, (X,), MeanFieldGuide(lri), (X,),
                                            {"w_loc": np.zeros(3), "w_std_log": np.zeros(3), "intercept_loc": 0.0})
    with pytest.raises(ValueError):
        M.sample_posterior_predictive(key, lri, (X,), AutoDiagonalNormal(lri), (X,), None)
    with pytest.raises(ValueError):     # substituted value of the wrong size
        M.sample_prior_predictive(key, lri, (X,), {"w": np.zeros(5)})
    with pytest.raises(ValueError):     # not a site of the model
        M.sample_prior_predictive(key, lri, (X,), {"mu": np.zeros(3)})
    vae = VAEModel(4, 8)
    with pytest.raises(ValueError, match="decoder"):
        M.sample_prior_predictive(key, vae, (2, 4, 8, 6))
    with pytest.raises(ValueError):
        M.sample_prior_predictive(key, vae, (2, 4, 8, 6), {"decoder$params": [(np.zeros((4, 8)), np.zeros(8)), (),
                                                                            (np.zeros((8, 5)), np.zeros(5)), ()]})


@pytest.mark.parametrize("bad", [None, np.zeros(2, np.uint32), torch.zeros(2, dtype=torch.int32), torch.zeros(3, dtype=torch.int32),
                                 torch.zeros(2, dtype=torch.float64), [0, 1]])
def test_a_key_that_is_not_a_two_word_cuda_tensor_raises_type_error(bad):
    X = np.zeros((10, 3), np.float32)
    lr = LogisticRegression(3)
    with pytest.raises(TypeError, match="threefry"):
        M.sample_prior_predictive(bad, lr, (X,))
    with pytest.raises(TypeError):
        M.sample_multi_posterior_predictive(bad, 2, lr, (X,), AutoDiagonalNormal(lr), (X,), {"auto_loc": np.zeros(3), "auto_scale": np.ones(3)})
