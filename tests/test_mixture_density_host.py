"""d3p_amd.mixture_density (held-out log predictive density and responsibilities of the mixture model), host side: the calibration
of the bound and the slack tests/test_gpu_mixture_density.py uses (tests/mixture_density_ref.py), the non-vacuity of the soft inputs,
the module surface and the C entries' declarations, every refusal before a device is touched, and the packed-view detection."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from . import mixture_density_ref as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def no_device(monkeypatch):
    import d3p_amd._lib as L

    def refuse(*a, **k):
        raise AssertionError("mixture_density reached require_device")
    monkeypatch.setattr(L, "require_device", refuse)


def _mg():
    from d3p_amd.models import GaussianMixtureGuide, GaussianMixtureModel
    m = GaussianMixtureModel()
    return m, GaussianMixtureGuide(m)


def test_module_surface_and_entry_points():
    import d3p_amd
    import d3p_amd._lib as L
    from d3p_amd import mixture_density as MD
    assert d3p_amd.mixture_density is MD and "mixture_density" in d3p_amd.__all__
    assert MD.__all__ == ["log_likelihood", "log_predictive_density", "responsibilities", "posterior_log_predictive_density",
                          "posterior_responsibilities", "posterior_summary", "ROW_TILE", "DRAW_TILE"]
    for name in MD.__all__[:6]:
        assert callable(getattr(MD, name))
    with open(os.path.join(ROOT, "include", "d3p_hip.h")) as f:
        hdr = f.read()
    for name in ("d3p_gmm_loglik_rows", "d3p_gmm_loglik_reduce"):
        assert re.search(r"\bint " + name + r"\(", hdr) and name in L.SIGNATURES, name
    assert re.search(r"#define D3P_ABI_VERSION 9\b", hdr)
    with open(os.path.join(ROOT, "d3p_amd", "csrc", "d3p_gmm_density.hip")) as f:
        src = f.read()
    assert MD.ROW_TILE == int(re.search(r"#define D3P_GD_ROW_TILE (\d+)", src).group(1))
    assert MD.DRAW_TILE == int(re.search(r"#define D3P_GD_DRAW_TILE (\d+)", src).group(1))
    assert int(re.search(r"#define D3P_GD_LDS_MAX (\d+)", src).group(1)) == 163840   # (draw_waves restates the rule with this figure)
    assert any(os.path.basename(p) == "d3p_gmm_density.hip" for p in L._SRC)
    lib = L.load()
    assert lib.d3p_abi_version() == 9 and hasattr(lib, "d3p_gmm_loglik_rows") and hasattr(lib, "d3p_gmm_loglik_reduce")


def test_import_stays_lazy():
    code = "import sys, d3p_amd; assert 'torch' not in sys.modules and 'd3p_amd.mixture_density' not in sys.modules; " \
           "d3p_amd.mixture_density; assert 'd3p_amd.mixture_density' in sys.modules"
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)


def test_infer_util_and_mixture_stay_as_they_were():
    from d3p_amd import infer_util as U
    from d3p_amd import mixture as MX
    m, _ = _mg()
    with pytest.raises(TypeError):
        U.log_likelihood(m, {"pis": np.ones((1, 3))}, np.zeros((4, 2), np.float32))
    assert MX.__all__ == ["prior_predictive_samples", "posterior_predictive_samples", "assignment_log_posterior", "assign",
                          "compute_assignment_accuracy", "ROW_TILE"]


def test_draw_split_rule_at_the_shapes():
    """Four waves split the draws except at the two largest shapes, where four latent copies do not fit in a compute unit's LDS."""
    assert [D.draw_waves(k, d) for k, d in ((3, 2), (16, 64), (16, 128), (32, 64), (16, 256), (32, 128))] == [4, 4, 4, 4, 2, 2]
    for k, d in ((16, 256), (32, 128), (1, 256), (32, 1)):
        W = D.draw_waves(k, d)
        stage = 4 * (((D.T * (d | 1) + 1) & ~1) + W * (2 * k * d + ((k + 1) & ~1)))
        assert stage <= 163840 and 64 * 8 * (k + 1) + 256 <= 163840, (k, d)


# ------------------------------------------------------------------------------------------------ calibration and non-vacuity
def test_bound_and_slack_calibration():
    """The numpy float32 restatement of k_gmm_density's operation order against the float64 comparator over the GPU tests' inputs,
    and the restated reduction against the float64 reduction of the same float32 a: the largest errors are what
    tests/mixture_density_ref.py records, and the bound and the slack are four times them."""
    worst_a, worst_s = 0.0, 0.0
    for kind in D.KINDS:
        for case in D.CASES:
            ea, es = D.errors_of_case(kind, *case)
            print(f"{kind} k, d, rows, n = {case}: a {ea:.3f} ulps of scale, reduction {es:.3f} slack units")
            worst_a, worst_s = max(worst_a, ea), max(worst_s, es)
    print(f"largest: a {worst_a:.3f}, reduction {worst_s:.3f}")
    assert 0.9 * D.A_ERR_SEEN_ULPS <= worst_a <= D.A_ERR_SEEN_ULPS, worst_a   # (the record is what the run gives)
    assert 0.9 * D.SLACK_ERR_SEEN_ULPS <= worst_s <= D.SLACK_ERR_SEEN_ULPS, worst_s
    assert D.BOUND_ULPS == pytest.approx(4 * D.A_ERR_SEEN_ULPS, rel=1e-3)
    assert D.SLACK_ULPS == pytest.approx(4 * D.SLACK_ERR_SEEN_ULPS, rel=1e-3)


def test_restatement_lies_inside_its_own_intervals():
    """The float32 restatement, taken as a stand-in for the device, passes the checks the GPU test applies."""
    for kind in D.KINDS:
        for case in D.CASES:
            ref = D.reference(kind, *case)
            a32 = D.a32_restated(ref["obs"], ref["pis"], ref["mus"], ref["sigs"])
            assert np.all(np.abs(a32 - ref["a"]) <= ref["b"])
            ll32, p32 = D.ll32_restated(a32)
            W = D.draw_waves(case[0], case[1])
            assert np.all((ll32 >= ref["ll_lo"]) & (ll32 <= ref["ll_hi"]))
            lp = D.lppd32_restated(ll32, W)
            assert np.all((lp >= ref["lppd_lo"]) & (lp <= ref["lppd_hi"]))
            rs = D.resp32_restated(p32, W)
            assert np.all((rs >= ref["resp_lo"]) & (rs <= ref["resp_hi"]))


def test_soft_inputs_are_soft_and_their_intervals_tight():
    """Non-vacuity, from the float64 reference alone: on soft_inputs at every test shape with k >= 2 at least half the rows have a
    maximum responsibility below 0.9, and at most 10 % of the (r, j) intervals are wider than 1e-3.  The hard inputs are near
    one-hot, which is what they are for."""
    for case in D.CASES:
        k = case[0]
        if k < 2:
            continue
        ref = D.reference("soft", *case)
        soft_rows = float((ref["resp"].max(axis=1) < 0.9).mean())
        wide = float(((ref["resp_hi"] - ref["resp_lo"]) > 1e-3).mean())
        print(f"soft k, d, rows, n = {case}: rows with max resp < 0.9: {soft_rows:.3f}; intervals wider than 1e-3: {wide:.3f}")
        assert soft_rows >= 0.5, case
        assert wide <= 0.10, case
        assert np.allclose(ref["resp"].sum(axis=1), 1.0, atol=1e-12)
    hard = D.reference("hard", 3, 2, D.T + 1, 2)
    assert float((hard["resp"].max(axis=1) > 0.999).mean()) > 0.9


def test_interval_helpers():
    assert D.lse(np.array([[-np.inf, -np.inf]]), 1)[0] == -np.inf
    assert D.lse(np.array([[0.0, -np.inf]]), 1)[0] == 0.0
    assert D.lse(np.array([[1000.0, 1000.0]]), 1)[0] == pytest.approx(1000.0 + np.log(2.0))
    one = D.intervals(np.zeros((2, 1), np.float32), np.ones((1, 1), np.float32), np.zeros((1, 1, 1), np.float32), np.ones((1, 1, 1), np.float32))
    assert np.all(one["resp"] == 1.0) and np.all(one["resp_lo"] <= 1.0) and np.all(one["resp_hi"] >= 1.0)
    assert one["ll"][0, 0] == pytest.approx(-D.HALF_LOG_2PI)


# ------------------------------------------------------------------------------------------------ refusals
def test_every_refusal_comes_before_the_device(no_device):
    from d3p_amd import mixture_density as MD
    from d3p_amd.models import AutoDiagonalNormal, LogisticRegression
    m, g = _mg()
    lr = LogisticRegression(2)
    key = torch.zeros(2, dtype=torch.int32)   # (a CPU tensor: not a threefry CUDA key)
    obs = np.zeros((10, 2), np.float32)
    args = (3, obs, 10, 2)
    params = {"alpha_log": np.zeros(3, np.float32), "mus_loc": np.zeros((3, 2), np.float32)}
    good = {"pis": np.full((4, 3), 1 / 3, np.float32), "mus": np.zeros((4, 3, 2), np.float32), "sigs": np.ones((4, 3, 2), np.float32)}
    direct = (MD.log_likelihood, MD.log_predictive_density, MD.responsibilities)
    post = (MD.posterior_log_predictive_density, MD.posterior_responsibilities, MD.posterior_summary)
    for fn in direct:
        with pytest.raises(TypeError):
            fn(lr, good, obs)
        for bad in (None, {"pis": good["pis"], "mus": good["mus"]},                                  # not a dict, a site missing
                    dict(good, pis=good["pis"][0]),                                                  # no leading axis
                    dict(good, mus=good["mus"][0]), dict(good, mus=good["mus"][:3]), dict(good, mus=np.zeros((4, 2, 2), np.float32)),
                    dict(good, sigs=np.ones((4, 3, 3), np.float32)), dict(good, sigs=np.ones((3, 3, 2), np.float32)),
                    {"pis": np.zeros((0, 3), np.float32), "mus": np.zeros((0, 3, 2), np.float32), "sigs": np.ones((1, 1, 1), np.float32)}):
            with pytest.raises(ValueError):
                fn(m, bad, obs)
        for bad_obs in (None, obs[0], np.zeros((10, 3), np.float32)):
            with pytest.raises(ValueError):
                fn(m, good, bad_obs)
        for k, d in ((17, 256), (33, 1), (1, 257), (32, 129)):
            big = {"pis": np.ones((1, k), np.float32), "mus": np.zeros((1, k, d), np.float32), "sigs": np.ones((1, 1, 1), np.float32)}
            with pytest.raises(ValueError):
                fn(m, big, np.zeros((2, d), np.float32))
    for fn in post:
        with pytest.raises(TypeError):
            fn(key, 2, lr, args, g, params)
        with pytest.raises(TypeError):
            fn(key, 2, m, args, AutoDiagonalNormal(lr), params)
        with pytest.raises(TypeError):
            fn(key, 2, m, args, None, params)
        for bad_n in (0, -1, None):
            with pytest.raises(ValueError):
                fn(key, bad_n, m, args, g, params)
        with pytest.raises(ValueError):
            fn(key, 2, m, (3, None, 10, 2), g, params)                     # obs is required: its values are scored
        with pytest.raises(ValueError):
            fn(key, 2, m, (3, obs[0]), g, params)
        with pytest.raises(NotImplementedError):
            fn(key, 2, m, (3, obs, 11), g, params)                         # plate mismatch, as d3p_amd.mixture
        for k, d in ((17, 256), (33, 1), (1, 257), (32, 129), (0, 2)):
            with pytest.raises(ValueError):
                fn(key, 2, m, (k, np.zeros((4, d), np.float32)), g, params)
        for bad in (None, {"alpha_log": np.zeros(3)}, {"alpha_log": np.zeros(4), "mus_loc": np.zeros((3, 2))},
                    {"alpha_log": np.zeros(3), "mus_loc": np.zeros((2, 3))}):
            with pytest.raises(ValueError):
                fn(key, 2, m, args, g, bad)
        for bad_key in (key, None, torch.zeros(3, dtype=torch.int32), np.zeros(2, np.uint32)):   # the key's type is the last host check
            with pytest.raises(TypeError):
                fn(bad_key, 2, m, args, g, params)


# ------------------------------------------------------------------------------------------------ packed views
def test_packed_view_detection_on_cpu_tensors():
    from d3p_amd import mixture_density as MD
    cpu = torch.device("cpu")
    n, k, d = 3, 2, 5
    kd, ld = k * d, k + 2 * k * d
    buf = torch.arange(n * ld, dtype=torch.float32).reshape(n, ld)

    def views(b, off=0):
        return (b[:, off:off + k], b[:, off + k:off + k + kd].unflatten(1, (k, d)),
                b[:, off + k + kd:off + k + 2 * kd].unflatten(1, (k, d)))

    pis, mus, sigs = views(buf)
    got = MD._packed_view(pis, mus, sigs, n, k, d, cpu)
    assert got is not None and got[0].data_ptr() == buf.data_ptr() and got[1] == ld
    # a wider buffer with the latents at an offset: read in place with its leading dimension
    wide = torch.zeros((n, ld + 7))
    p2, m2, s2 = views(wide, off=3)
    got = MD._packed_view(p2, m2, s2, n, k, d, cpu)
    assert got is not None and got[0].data_ptr() == wide.data_ptr() + 3 * 4 and got[1] == ld + 7
    # one draw: the leading dimension is the row's own length
    got = MD._packed_view(pis[:1], mus[:1], sigs[:1], 1, k, d, cpu)
    assert got is not None and got[1] == ld
    # everything else is packed: another storage, another order, another dtype, a transposed or expanded site, another device
    assert MD._packed_view(pis.clone(), mus, sigs, n, k, d, cpu) is None
    assert MD._packed_view(pis, sigs, mus, n, k, d, cpu) is None
    assert MD._packed_view(pis.double(), mus.double(), sigs.double(), n, k, d, cpu) is None
    assert MD._packed_view(pis, mus, sigs[:, :1].expand(n, k, d), n, k, d, cpu) is None
    assert MD._packed_view(pis, mus.transpose(1, 2), sigs, n, d, k, cpu) is None
    assert MD._packed_view(pis[::2], mus[::2], sigs[::2], 2, k, d, cpu) is not None      # (every other row: ld doubles, still a view)
    assert MD._packed_view(pis[::2], mus[::2], sigs[::2], 2, k, d, cpu)[1] == 2 * ld
    assert MD._packed_view(pis, mus, sigs, n, k, d, torch.device("meta")) is None
    assert MD._packed_view(pis.numpy(), mus, sigs, n, k, d, cpu) is None
