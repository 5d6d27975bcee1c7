"""d3p_amd._tables without a GPU: every shared check has one definition, a table diagnostic does not import the model stack, and
every public function of the table family makes its argument checks, then asks the device question, and reaches no device on the way."""
import glob
import inspect
import os
import subprocess
import sys

import pytest
import torch

import d3p_amd._lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODULES = ("fidelity", "permutation", "neighbours", "marginals", "covariance", "univariate", "mixed", "sliced", "mmd", "sinkhorn", "energy")

ONCE = ("one dtype for both tables", "the tables lie on different devices", "exclude_diagonal must be a bool", "compares a table with itself",
        "int32 values beyond 2^24 in magnitude: the kernel converts", "the rows of the tensor overlap", "at most 2^31 - 1 are sorted",
        "m2.diagonal()", "== torch.float32 else 1")


def test_every_shared_check_has_one_definition():
    texts = {}
    for path in glob.glob(os.path.join(ROOT, "d3p_amd", "*.py")):
        with open(path) as f:
            texts[os.path.basename(path)] = f.read()
    for needle in ONCE:
        assert sum(needle in t for t in texts.values()) == 1, (needle, sorted(n for n, t in texts.items() if needle in t))


def test_a_table_diagnostic_does_not_import_the_model_stack():
    code = "import sys, d3p_amd.covariance; " \
           "assert not {'d3p_amd.energy', 'd3p_amd.models', 'd3p_amd.mixture'} & set(sys.modules), sorted(m for m in sys.modules if 'd3p' in m)"
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)


# public names that take no table, so have no device question to ask: host-only arithmetic, constants of the library, and the one
# function whose draws come from mixture.posterior_predictive_samples (that entry asks it)
NO_TABLE = {("permutation", "permutation_labels"), ("neighbours", "max_k"), ("sliced", "random_directions"), ("energy", "draws_limit"),
            ("energy", "compare_energy_scores"), ("energy", "posterior_predictive_energy_score")}


def _calls():
    """(module, function, args, kwargs, malformed args, malformed kwargs, the malformed argument's message), one row per public name:
    3 rows by 2 columns, a holdout where the function takes one."""
    from d3p_amd import marginals as MG
    from d3p_amd import mixed as MX
    x, xi, wide = torch.zeros((3, 2)), torch.zeros((3, 2), dtype=torch.int32), torch.zeros((3, 3))
    v3, labels = torch.zeros(3), torch.zeros((1, 1), dtype=torch.uint32)
    edges = MG.bin_edges(x, [[0.0], [0.0]])
    schema, schema3 = MX.MixedSchema((0, 0), (1.0, 1.0), 0.0, 2.0, (1.0, 1.0)), MX.MixedSchema((0,) * 3, (1.0,) * 3, 0.0, 3.0, (1.0,) * 3)
    theta, s, draws = torch.zeros((2, 1)), torch.zeros((2, 3)), torch.zeros((3, 3, 2))
    return [
        ("fidelity", "pair_stats", (x, x), {}, (x, x, 2), {}, "exclude_diagonal must be a bool"),
        ("fidelity", "energy_distance", (x, x), {}, (x, wide), {}, "x has 2 columns and y has 3"),
        ("fidelity", "closest_record", (x, x), {}, (x, xi), {}, "synthetic is torch.float32 and real is torch.int32"),
        ("fidelity", "fidelity_report", (x, x, x), {}, (x, x, wide), {}, "holdout has 3 columns and synthetic has 2"),
        ("permutation", "label_sums", (x, labels), {}, (x, labels, v3), {}, "row_sum: a contiguous float64"),
        ("permutation", "energy_test", (x, x, 3), {}, (x, x, 0), {}, "n_perm must be an int >= 1"),
        ("neighbours", "knn", (x, x, 1), {}, (x, x, 0), {}, "k must be an int in"),
        ("neighbours", "kth_neighbour", (x, 1), {}, (x, True), {}, "k must be an int in"),
        ("neighbours", "ball_counts", (x, x, v3), {}, (x, x, torch.zeros(2)), {}, "radius_sq: a 1-D float32"),
        ("neighbours", "prdc", (x, x, 2, x), {}, (x, x, 2, wide), {}, "holdout has 3 columns and real has 2"),
        ("marginals", "bin_edges", (x,), {}, (x, 0), {}, "bins must be an int in"),
        ("marginals", "marginal_counts", (x, edges), {}, (x, None), {}, "edges: a BinEdges"),
        ("marginals", "marginal_fidelity", (x, x), {"holdout": x}, (x, x), {"top": -1}, "top must be a non-negative int"),
        ("covariance", "column_moments", (x,), {}, (torch.zeros((3, 0)),), {}, "d >= 1 is required"),
        ("covariance", "covariance", (x,), {}, (x, 3), {}, "ddof must be an int in"),
        ("covariance", "correlation", (x,), {}, (torch.zeros((0, 2)),), {}, "at least one row"),
        ("covariance", "correlation_fidelity", (x, x, x), {}, (x, x, wide), {}, "holdout has 3 columns and real has 2"),
        ("univariate", "sort_columns", (x,), {}, (torch.zeros((2, 3)).t(),), {}, "the columns must have unit stride"),
        ("univariate", "midranks", (x,), {}, (torch.zeros(2).expand(3, 2),), {}, "the rows of the tensor overlap"),
        ("univariate", "spearman", (x,), {}, (torch.zeros((3, 0)),), {}, "d >= 1 is required"),
        ("univariate", "cdf_distance", (x, x), {}, (x, xi), {}, "one dtype for both tables"),
        ("univariate", "univariate_fidelity", (x, x, x), {}, (x, x, x), {"top": True}, "top must be a non-negative int"),
        ("mixed", "mixed_schema", (x, [0]), {}, (x, [2]), {}, "categorical: an index outside"),
        ("mixed", "pair_stats", (x, x, schema), {}, (x, x, schema, 2), {}, "exclude_diagonal must be a bool"),
        ("mixed", "energy_distance", (x, x, schema), {}, (x, x, schema3), {}, "the schema has 3 columns and the tables 2"),
        ("mixed", "closest_record", (x, x, schema), {}, (x, x, None), {}, "schema: a MixedSchema"),
        ("sliced", "project", (x, theta), {}, (x, theta, v3), {}, r"shift must be None or a contiguous float32 tensor of shape \(2,\)"),
        ("sliced", "w2_distance", (s, s), {}, (s, wide), {}, "sa has 2 columns and sb has 3"),
        ("sliced", "sliced_wasserstein", (x, x), {"n_dirs": 2, "holdout": x}, (x, x), {"n_dirs": 0}, "n_dirs must be an int >= 1"),
        ("mmd", "kernel_sums", (x, x, 1.0), {}, (x, x, 0.0), {}, "gamma0 must be a finite number > 0"),
        ("mmd", "mmd", (x, x), {}, (x, x), {"scale": "iqr"}, "scale must be 'std' or None"),
        ("sinkhorn", "softmin_rows", (x, x, 1.0, v3), {}, (x, x, 1.0, torch.zeros(2)), {}, "h must be a contiguous float32"),
        ("sinkhorn", "sinkhorn_divergence", (x, x), {}, (x, x), {"check_every": 0}, "check_every must be an int >= 1"),
        ("energy", "energy_score_draws", (draws, x), {}, (draws, torch.zeros((2, 2))), {}, r"y: shape \(3, 2\) expected"),
        ("energy", "energy_score", (draws, x), {}, (draws, torch.zeros((2, 2))), {}, r"y: shape \(3, 2\) expected"),
    ]


def test_every_public_function_checks_its_arguments_then_asks_for_a_device(monkeypatch):
    import importlib

    def reached():
        raise AssertionError("a host check reached require_device")
    monkeypatch.setattr(L, "require_device", reached)
    calls = _calls()
    public = {(m, n) for m in MODULES for n in importlib.import_module("d3p_amd." + m).__all__
              if inspect.isfunction(getattr(importlib.import_module("d3p_amd." + m), n))}
    assert {(m, n) for m, n, *_ in calls} | NO_TABLE == public and len(calls) + len(NO_TABLE) == len(public)
    for module, name, args, kw, bad_args, bad_kw, match in calls:
        fn = getattr(importlib.import_module("d3p_amd." + module), name)
        with pytest.raises(ValueError, match=r"CUDA tensor .* is required"):
            fn(*args, **kw)
        with pytest.raises(ValueError, match=match):
            fn(*bad_args, **bad_kw)
