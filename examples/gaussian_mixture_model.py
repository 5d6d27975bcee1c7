#!/usr/bin/env python3
"""Gaussian mixture model with DP-VI on MI355X -- the workload of the reference's
examples/gaussian_mixture_model.py (BASELINE config 3): model :51-68 (Dirichlet weights, Normal(0, 10) means,
InverseGamma(1, 1) scales, d3p.gmm.GaussianMixture likelihood), guide :70-85 (alpha_log, mus_loc), three-cluster toy data
:87-110, Poisson-subsampled training with clipping threshold 20 :176-232, and the final report of the learned mixture
weights and modes plus the cluster-assignment accuracy on held-out data :112-161.

Differences to the reference script, forced by the environment: model and guide are declared
(d3p_amd.models.GaussianMixtureModel / GaussianMixtureGuide) instead of traced NumPyro functions, the toy data comes
from torch's generator, dp_scale is calibrated for --epsilon by d3p_amd.dputil as in the reference (:193-196), or given directly with --sigma.

Two opt-in flags follow the reference where the defaults deviate from it (d3p_amd.mixture): --toy-data predictive makes the data as
the reference does, with the prior predictive and the three latent sites substituted (:87-108); --assignment posterior scores with
the reference's compute_assignment_accuracy on the per-component log-posterior -- unit scales, the learned weights, the inverse mode
map (:113-161) -- instead of the closest mode.

--held-out-density (off by default; d3p_amd.mixture_density) adds two lines after training: the mean log predictive density of the
test split under --posterior-draws draws from the fitted guide, and the accuracy of the argmax of the responsibilities averaged over
the same draws, beside the assignment accuracy above.

--waic (off by default; d3p_amd.criteria) adds one line: elpd_waic +- its standard error and p_waic of the fitted mixture on the
training split, under --posterior-draws draws from the fitted guide.

--loo (off by default; d3p_amd.criteria) adds one line: the PSIS-LOO elpd_loo +- its standard error, p_loo and the number of points
whose Pareto shape lies above the threshold, on the same split and draws.

--guide-diagnostic [N_DRAWS] (off by default; d3p_amd.mixture_diagnostics) adds one line: the full-data ELBO +- its standard error, the
importance-sampling estimate of the log evidence, the Pareto k of the guide's importance ratios against its threshold and their
effective sample size, on the training split (Yao et al. 2018: is the trained guide a usable approximation of the posterior?).

--energy-score [N_DRAWS] (off by default; d3p_amd.energy) adds one line beside --held-out-density: the energy score (the multivariate
CRPS, Gneiting & Raftery 2007) of N_DRAWS posterior predictive draws per point of the test split +- its standard error, with its two
parts, the mean distance of a draw to the point and the spread of the draws.  It scores the draws a user would ship as synthetic data,
in the data's own units; smaller is better.

--synthetic-fidelity (off by default; d3p_amd.fidelity) draws ONE synthetic table of the training split's size from the posterior
predictive and adds two lines: its energy distance (Szekely & Rizzo) to the training and to the test split, and the quantiles of the
distance to the closest training record, the number of exact copies, the nearest-neighbour adversarial accuracy (Yale et al. 2020; 0.5:
indistinguishable) against the training and the held-out split and their difference, the privacy loss.  The numbers are functions of
the private table and are not covered by the accountant.

--marginal-fidelity [BINS] (off by default; d3p_amd.marginals) draws the same synthetic table and adds two lines of its own: the mean
and the worst total variation distance of the binned one-way marginals (BINS quantile bins of the training split, default 16) and of
the two-way marginals with the worst pair of columns, and the mean and largest difference of the pairwise associations (Cramer's V),
followed by the floor -- what the test split, a fresh sample of the same distribution, scores against the training split.  These too
are functions of the private table and are not covered by the accountant.

--energy-test [N_PERM] (off by default; d3p_amd.permutation) draws the same synthetic table and adds one line: the permutation test of
its energy distance (Szekely & Rizzo; N_PERM relabellings of the pooled rows, default 199) against the training and against the test
split -- the statistic, its p-value and the 95 % quantile of the relabelled statistics.  A function of the private table too, not
covered by the accountant; with many rows it rejects at differences too small to matter, so read it beside --synthetic-fidelity's d2.
"""
import argparse
import itertools
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import d3p_amd._lib as L  # noqa: E402
import d3p_amd.random as rng_suite  # noqa: E402
from d3p_amd.minibatch import poisson_batchify_data, split_batchify_data  # noqa: E402
from d3p_amd.models import Adam, GaussianMixtureGuide, GaussianMixtureModel, Trace_ELBO  # noqa: E402
from d3p_amd.svi import DPSVI  # noqa: E402


def create_toy_data(N, d, seed=1234):
    """Imbalanced three-component data: the last component has twice as many samples (reference :87-110)."""
    g = torch.Generator().manual_seed(seed)
    mus = torch.tensor([-10.0, 10.0, -2.0])
    sigs = torch.tensor([0.1, 1.0, 0.1])
    z = torch.multinomial(torch.tensor([0.25, 0.25, 0.5]), 2 * N, replacement=True, generator=g)
    X = mus[z, None] + sigs[z, None] * torch.randn(2 * N, d, generator=g)
    X, z = X.cuda(), z.cuda()
    return X[:N].contiguous(), X[N:].contiguous(), z[N:], mus.cuda()


def create_toy_data_predictive(N, d, seed=1234):
    """The reference's create_toy_data (:87-108): one prior predictive draw of 2 N rows with pis, mus and sigs substituted; the
    component of every row comes back as the intermediate of `obs`."""
    from d3p_amd import mixture
    from d3p_amd.random import debug as threefry   # (a jax.random key in the reference)
    mus = torch.tensor([-10.0, 10.0, -2.0])
    samples = mixture.prior_predictive_samples(threefry.PRNGKey(seed), None, GaussianMixtureModel(), (3, None, 2 * N, d), substitutes={
        "pis": torch.tensor([0.25, 0.25, 0.5]), "mus": mus[:, None].expand(-1, d), "sigs": torch.tensor([[0.1], [1.0], [0.1]])
    }, with_intermediates=True)
    X, z = samples["obs"][0], samples["obs"][1][0]
    return X[:N].contiguous(), X[N:].contiguous(), z[N:], mus.cuda()


def assignment_accuracy(X_test, z_test, true_mus, modes):
    """Assign every held-out point to the closest learned mode, map learned modes to true components by the best
    permutation and compare with the generating assignment (reference :112-161, with unit scales)."""
    k = modes.shape[0]
    assign = torch.cdist(X_test, modes).argmin(dim=1)
    d = X_test.shape[1]
    centres = true_mus[:, None].expand(-1, d)
    best = 0.0
    for perm in itertools.permutations(range(k), centres.shape[0]):
        # perm[j] = learned component standing for true component j
        mapped = torch.full((k,), -1, device=X_test.device, dtype=torch.long)
        for j, c in enumerate(perm):
            mapped[c] = j
        best = max(best, float((mapped[assign] == z_test).float().mean()))
    return best


def held_out_density(X_test, z_test, params, k, num_draws, seed=4321):
    """(mean log predictive density of X_test, accuracy of the argmax of the posterior-averaged responsibilities under the best map
    of learned components to true ones) under num_draws draws from the guide at params -- one pass over the draws."""
    from d3p_amd import mixture_density
    from d3p_amd.random import debug as threefry
    model = GaussianMixtureModel()
    out = mixture_density.posterior_summary(threefry.PRNGKey(seed), num_draws, model, (k, X_test), GaussianMixtureGuide(model), params)
    soft = out["responsibilities"].argmax(dim=1)
    n_true = int(z_test.max()) + 1
    best = 0.0
    for perm in itertools.permutations(range(k), n_true):
        mapped = torch.full((k,), -1, device=soft.device, dtype=torch.long)
        for j, c in enumerate(perm):
            mapped[c] = j
        best = max(best, float((mapped[soft] == z_test).float().mean()))
    return float(out["log_predictive_density"].mean()), best


def energy_score_report(X_test, params, k, num_draws, seed=4324):
    """The EnergyScoreResult of num_draws posterior predictive draws per held-out point against X_test (d3p_amd.energy): the
    multivariate CRPS, in the data's own units."""
    from d3p_amd import energy
    from d3p_amd.random import debug as threefry
    model = GaussianMixtureModel()
    return energy.posterior_predictive_energy_score(threefry.PRNGKey(seed), num_draws, model, (k, X_test), GaussianMixtureGuide(model), params)


def synthetic_fidelity_report(X_train, X_test, params, k, seed=4325):
    """The FidelityReport (d3p_amd.fidelity) of one synthetic table of X_train's size -- one posterior predictive draw per row --
    against the training split, with the test split as the holdout."""
    from d3p_amd import fidelity, mixture
    from d3p_amd.random import debug as threefry
    model = GaussianMixtureModel()
    synthetic = mixture.posterior_predictive_samples(threefry.PRNGKey(seed), 1, model, (k, X_train), GaussianMixtureGuide(model),
                                                     params)["obs"][0]
    return fidelity.fidelity_report(X_train, synthetic, holdout=X_test)


def marginal_fidelity_report(X_train, X_test, params, k, bins, seed=4325):
    """The MarginalFidelity (d3p_amd.marginals) of the synthetic table of synthetic_fidelity_report against the training split, cut at
    the training split's quantiles into `bins` bins, with the test split as the holdout (the noise floor)."""
    from d3p_amd import marginals, mixture
    from d3p_amd.random import debug as threefry
    model = GaussianMixtureModel()
    synthetic = mixture.posterior_predictive_samples(threefry.PRNGKey(seed), 1, model, (k, X_train), GaussianMixtureGuide(model),
                                                     params)["obs"][0]
    return marginals.marginal_fidelity(X_train, synthetic, bins=bins, holdout=X_test)


def energy_test_report(X_train, X_test, params, k, n_perm, seed=4325):
    """The EnergyTests (d3p_amd.permutation) of the synthetic table of synthetic_fidelity_report against the training and against the
    test split, n_perm relabellings each."""
    from d3p_amd import mixture, permutation
    from d3p_amd.random import debug as threefry
    model = GaussianMixtureModel()
    synthetic = mixture.posterior_predictive_samples(threefry.PRNGKey(seed), 1, model, (k, X_train), GaussianMixtureGuide(model),
                                                     params)["obs"][0]
    return permutation.energy_test(synthetic, X_train, n_perm=n_perm), permutation.energy_test(synthetic, X_test, n_perm=n_perm)


def waic_report(X, params, k, num_draws, seed=4322):
    """The WAICResult of the fitted mixture on X under num_draws draws from the guide at params."""
    from d3p_amd import criteria
    from d3p_amd.random import debug as threefry
    model = GaussianMixtureModel()
    return criteria.posterior_waic(threefry.PRNGKey(seed), num_draws, model, (k, X), GaussianMixtureGuide(model), params)


def loo_report(X, params, k, num_draws, seed=4322):
    """The LOOResult of the fitted mixture on X on waic_report's draws."""
    from d3p_amd import criteria
    from d3p_amd.random import debug as threefry
    model = GaussianMixtureModel()
    return criteria.posterior_loo(threefry.PRNGKey(seed), num_draws, model, (k, X), GaussianMixtureGuide(model), params)


def guide_diagnostic_report(X, params, k, num_draws, seed=4323):
    """The guide diagnostic line (d3p_amd.mixture_diagnostics): ELBO, importance-sampling evidence, Pareto k and effective sample
    size of num_draws draws from the guide at params on the whole table X."""
    from d3p_amd import mixture_diagnostics
    from d3p_amd.random import debug as threefry
    model = GaussianMixtureModel()
    res = mixture_diagnostics.guide_diagnostic(threefry.PRNGKey(seed), num_draws, model, (k, X), GaussianMixtureGuide(model), params)
    return ("guide diagnostic ({} rows, {} draws): elbo {:.2f} +- {:.2f}, log_evidence_is {:.2f}, pareto k {:.2f} (threshold {:.2f}), "
            "ess {:.1f}").format(res.n_rows, res.n_draws, float(res.elbo), float(res.elbo_se), float(res.log_evidence_is),
                                 float(res.pareto_k), res.k_threshold, float(res.ess))


def main(args):
    L.require_device()
    N, k, d = args.num_samples, args.num_components, args.dimensions
    q = args.batch_size / N
    if getattr(args, "toy_data", "torch") == "predictive":
        X_train, X_test, z_test, true_mus = create_toy_data_predictive(N, d)
    else:
        X_train, X_test, z_test, true_mus = create_toy_data(N, d)
    train_init, train_fetch = poisson_batchify_data((X_train,), q=q, max_batch_size=.99, rng_suite=rng_suite)
    test_init, test_fetch = split_batchify_data((X_test,), batch_size=args.batch_size, rng_suite=rng_suite)

    dpsvi_rng = rng_suite.PRNGKey(0)
    dpsvi_rng, svi_init_rng, fetch_rng = rng_suite.split(dpsvi_rng, 3)
    iters_per_epoch, batchifier_state = train_init(fetch_rng)

    dp_scale = getattr(args, "sigma", None)
    if dp_scale is None:  # examples/gaussian_mixture_model.py:193-196
        from d3p_amd.dputil import approximate_sigma_remove_relation
        # (maxeval 20 instead of the default 10: at epsilon = 10 the search starts next to the accountant's unstable
        # range and needs the extra evaluations to reach the tolerance; very few iterations -- e.g. -n 3 -- put the answer
        # inside that range and raise RuntimeError, as designed in d3p/dputil.py:69-70: pass --sigma then)
        dp_scale, eps, _ = approximate_sigma_remove_relation(args.epsilon, 1 / N, q, num_iter=iters_per_epoch * args.num_epochs,
                                                             maxeval=20)
        print("noise scale {:.4f} for epsilon {:.4f}, delta {:.2e}".format(dp_scale, eps, 1 / N))
    model = GaussianMixtureModel()
    svi = DPSVI(model, GaussianMixtureGuide(model), Adam(args.learning_rate), Trace_ELBO(), dp_scale=dp_scale,
                clipping_threshold=20., k=k, num_obs_total=N, rng_suite=rng_suite)
    batch, _ = train_fetch(0, batchifier_state)
    svi_state = svi.init(svi_init_rng, *batch)

    for i in range(args.num_epochs):
        t0 = time.time()
        dpsvi_rng, data_fetch_rng = rng_suite.split(dpsvi_rng, 2)
        num_batches, batchifier_state = train_init(rng_key=data_fetch_rng)
        losses = []
        for j in range(num_batches):
            batch, mask = train_fetch(j, batchifier_state)
            svi_state, batch_loss = svi.update(svi_state, *batch, mask=mask)
            losses.append(batch_loss)
        train_loss = float(torch.stack(losses).sum()) / (N * num_batches)
        t1 = time.time()
        if i % max(args.num_epochs // 5, 1) == 0:
            dpsvi_rng, test_fetch_rng = rng_suite.split(dpsvi_rng, 2)
            num_test_batches, test_state = test_init(rng_key=test_fetch_rng)
            test_loss = sum(float(svi.evaluate(svi_state, *test_fetch(j, test_state)))
                            for j in range(num_test_batches)) / (N * num_test_batches)
            print("Epoch {}: loss = {:.4f} (on training set = {:.4f}) ({:.2f} s.)".format(i, test_loss, train_loss, t1 - t0))

    params = svi.get_params(svi_state)
    modes = params["mus_loc"]
    alpha = torch.exp(params["alpha_log"])
    pis = alpha / alpha.sum()                     # mean of Dirichlet(alpha)
    print("MAP estimate of mixture weights: {}".format(pis.tolist()))
    print("MAP estimate of mixture modes  : {}".format(modes.tolist()))
    if getattr(args, "assignment", "modes") == "posterior":
        from d3p_amd.mixture import compute_assignment_accuracy
        acc = compute_assignment_accuracy(X_test, z_test, true_mus[:, None].expand(-1, d), modes, pis)
    else:
        acc = assignment_accuracy(X_test, z_test, true_mus, modes)
    print("assignment accuracy: {:.4f}".format(acc))
    if getattr(args, "held_out_density", False):
        lppd, soft_acc = held_out_density(X_test, z_test, params, k, args.posterior_draws)
        print("held-out log predictive density (mean over {} points, {} posterior draws): {:.4f}".format(
            X_test.shape[0], args.posterior_draws, lppd))
        print("assignment accuracy (argmax of posterior responsibilities): {:.4f}".format(soft_acc))
    if getattr(args, "energy_score", None) is not None:
        res = energy_score_report(X_test, params, k, args.energy_score)
        print("held-out energy score (mean over {} points, {} predictive draws): {:.4f} +- {:.4f} (mean distance {:.4f}, spread {:.4f})".format(
            res.n_rows, res.n_draws, float(res.es), float(res.se), float(res.mae), float(res.spread)))
    if getattr(args, "synthetic_fidelity", False):
        res = synthetic_fidelity_report(X_train, X_test, params, k)
        print("synthetic table ({} rows, d = {}): energy distance to train {:.5f} ({} rows), to test {:.5f} ({} rows)".format(
            res.n_synthetic, res.dim, float(res.energy_train.d2), res.n_train, float(res.energy_holdout.d2), res.n_holdout))
        print("distance to closest training record: quantiles {} {}, exact copies {}; adversarial accuracy train {:.4f}, held-out {:.4f}, "
              "privacy loss {:.4f}".format("/".join("{:g}%".format(100 * p) for p in res.dcr_probs),
                                           "/".join("{:.4f}".format(v) for v in res.dcr_quantiles), res.n_exact_copies, res.aa,
                                           res.aa_holdout, res.privacy_loss))
    if getattr(args, "marginal_fidelity", None) is not None:
        res = marginal_fidelity_report(X_train, X_test, params, k, args.marginal_fidelity)
        pair = lambda r: "columns {} and {} ({:.4f})".format(r.worst_pairs[0][0][0], r.worst_pairs[0][0][1], r.worst_pairs[0][1]) \
            if r.worst_pairs else "none"  # noqa: E731
        print("binned marginals ({} bins, {} columns, {} synthetic rows): 1-way TVD mean {:.4f}, worst column {} ({:.4f}); 2-way TVD mean "
              "{:.4f}, worst {}".format(args.marginal_fidelity, len(res.columns), res.n_synthetic, res.tvd_one_way_mean, res.worst_columns[0][0],
                                        res.worst_columns[0][1], res.tvd_two_way_mean, pair(res)))
        print("association (Cramer's V) difference mean {:.4f}, max {:.4f}; held-out floor ({} rows): 1-way TVD mean {:.4f}, 2-way TVD mean "
              "{:.4f}, association difference mean {:.4f}".format(res.assoc_diff_mean, res.assoc_diff_max, res.floor.n_synthetic,
                                                                  res.floor.tvd_one_way_mean, res.floor.tvd_two_way_mean,
                                                                  res.floor.assoc_diff_mean))
    if getattr(args, "energy_test", None) is not None:
        tr, te = energy_test_report(X_train, X_test, params, k, args.energy_test)
        print("energy distance permutation test ({} relabellings): to train statistic {:.4f}, p {:.4f} (null 95% {:.4f}); to test statistic "
              "{:.4f}, p {:.4f} (null 95% {:.4f})".format(tr.n_perm, float(tr.statistic), tr.p_value, tr.null_quantiles[1],
                                                          float(te.statistic), te.p_value, te.null_quantiles[1]))
    if getattr(args, "waic", False):
        res = waic_report(X_train, params, k, args.posterior_draws)
        print("WAIC ({} points, {} posterior draws): elpd_waic {:.2f} +- {:.2f}, p_waic {:.2f}".format(
            res.n_rows, res.n_draws, float(res.elpd_waic), float(res.se), float(res.p_waic)))
    if getattr(args, "loo", False):
        res = loo_report(X_train, params, k, args.posterior_draws)
        print("PSIS-LOO ({} points, {} posterior draws): elpd_loo {:.2f} +- {:.2f}, p_loo {:.2f}, pareto k above {:.2f} in {} points".format(
            res.n_rows, res.n_draws, float(res.elpd_loo), float(res.se), float(res.p_loo), res.k_threshold, int(res.n_high_k)))
    if getattr(args, "guide_diagnostic", None) is not None:
        print(guide_diagnostic_report(X_train, params, k, args.guide_diagnostic))
    return acc, pis, modes


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description="parse args")
    parser.add_argument('-n', '--num-epochs', default=100, type=int, help='number of training epochs')
    parser.add_argument('-lr', '--learning-rate', default=5.0e-2, type=float, help='learning rate')
    parser.add_argument('-batch-size', default=32, type=int, help='batch size')
    parser.add_argument('-d', '--dimensions', default=2, type=int, help='data dimension')
    parser.add_argument('-N', '--num-samples', default=2048, type=int, help='data samples count')
    parser.add_argument('-k', '--num-components', default=3, type=int, help='number of components in the mixture model')
    parser.add_argument('-e', '--epsilon', default=10., type=float, help='privacy parameter epsilon (delta = 1 / N)')
    parser.add_argument('--sigma', default=None, type=float, help='dp_scale of the Gaussian mechanism (overrides --epsilon)')
    parser.add_argument('--toy-data', default='torch', choices=['torch', 'predictive'],
                        help="'predictive': make the data with the prior predictive, as the reference does")
    parser.add_argument('--assignment', default='modes', choices=['modes', 'posterior'],
                        help="'posterior': score with the per-component log-posterior, as the reference does")
    parser.add_argument('--held-out-density', action='store_true',
                        help='report the held-out log predictive density and the soft-assignment accuracy under the fitted posterior')
    parser.add_argument('--posterior-draws', default=100, type=int, help='posterior draws for --held-out-density, --waic and --loo')
    parser.add_argument('--loo', action='store_true',
                        help='report the PSIS-LOO elpd_loo, its standard error, p_loo and the count of high Pareto shapes')
    parser.add_argument('--waic', action='store_true', help='report elpd_waic, its standard error and p_waic of the fitted mixture')
    parser.add_argument('--guide-diagnostic', nargs='?', const=100, default=None, type=int, metavar='N_DRAWS',
                        help='after training, report the ELBO, the importance-sampling evidence, the Pareto k and the effective sample '
                             'size of N_DRAWS (default 100) draws from the guide on the training table')
    parser.add_argument('--energy-score', nargs='?', const=100, default=None, type=int, metavar='N_DRAWS',
                        help='after training, report the energy score (the multivariate CRPS) of N_DRAWS (default 100) posterior '
                             'predictive draws per point of the test split')
    parser.add_argument('--synthetic-fidelity', action='store_true',
                        help='after training, draw one synthetic table of the training split\'s size and report its energy distance to the '
                             'train and test splits, the distance to the closest record and the nearest-neighbour adversarial accuracy')
    parser.add_argument('--marginal-fidelity', nargs='?', const=16, default=None, type=int, metavar='BINS',
                        help='after training, draw one synthetic table of the training split\'s size and report the total variation '
                             'distance of its binned one- and two-way marginals (BINS quantile bins of the training split, default 16) and '
                             'the difference of the pairwise associations, with the test split\'s scores as the noise floor')
    parser.add_argument('--energy-test', nargs='?', const=199, default=None, type=int, metavar='N_PERM',
                        help='after training, draw one synthetic table of the training split\'s size and report the permutation test of its '
                             'energy distance to the train and test splits (N_PERM relabellings, default 199): statistic, p-value and the '
                             'null 95 %% quantile')
    return parser.parse_args(argv)


if __name__ == "__main__":
    main(parse_args())
