#!/usr/bin/env python3
"""Logistic regression with DP-VI on MI355X -- the workload of the reference's
examples/logistic_regression.py (model :49-66, training loop :118-204) on the d3p_amd surface.

Differences to the reference script, all forced by the environment: the model is declared
(d3p_amd.models.LogisticRegression) instead of traced from a NumPyro function, and an epoch is one `run_steps` call (the
reference's jit(fori_loop(...)) at :149-160).  `--guide handwritten` is the script's OWN guide (:67-86: sample sites 'w' and
'intercept', four parameter leaves with exp scales, one perturbation key per leaf) through the five-stage composition;
`--guide auto` (default) is AutoDiagonalNormal (README.md:99) on the fused device-resident loop.  As in the reference (:135-137) dp_scale is calibrated for --epsilon, with
d3p_amd.dputil on the restated Fourier accountant; --sigma gives it directly.

--clipping-profile (off by default; d3p_amd.clipping) adds two lines after training: the quantiles of the per-example gradient norms of
the whole table at the trained parameters, the share of rows the script's clipping threshold (1.0) clips with the mean clip factor, and the
median norm as the suggested threshold (Abadi et al. 2016).  They are computed from the private table without noise.
--ppc [N_DRAWS] (off by default; d3p_amd.ppc) adds, after training, one line per statistic -- mean, sd, min, max, zeros -- of the
posterior predictive check on the training table: the statistic of the observed outcomes, its mean and central 90 % range over N_DRAWS
data sets replicated from the trained guide, and the tail shares p_ge = P(T(y_rep) >= T(y)) and p_le.  The replicated data sets are
reduced as they are drawn; they are never written.
--discrepancy [N_DRAWS] (off by default; d3p_amd.discrepancy) adds, after training, the realized-discrepancy check of Gelman, Meng &
Stern (1996) on the training table: per draw from the trained guide the Pearson chi-square of the observed outcomes and of that draw's
own replicate, the share p_ge of draws whose replicate is at least as far from the mean as the data, the dispersion chi2_obs / rows
(near 1 for labels the model explains), and the Bayesian R^2 (both kinds), RMSE and bias per draw.
--classification-report [N_DRAWS] (off by default; d3p_amd.classification; --guide auto) adds, after training, the classifier's own
numbers on the TEST table: the sampled accuracy of N_DRAWS posterior draws -- the number --predictive-accuracy prints, here with its sd
and 90 % interval over the draws and without the N_DRAWS x rows label matrix -- then accuracy, TPR, FPR and F1 of the predicted
probability at the threshold 0.5, and of the posterior mean probability the AUC with its certificate [auc_lo, auc_hi], the KS statistic
and the expected calibration error.  estimate_accuracy below stays as the stored-matrix comparator.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import d3p_amd._lib as L  # noqa: E402
import d3p_amd.random as rng_suite  # noqa: E402
from d3p_amd.minibatch import poisson_batchify_data, split_batchify_data  # noqa: E402
from d3p_amd.models import Adam, AutoDiagonalNormal, LogisticRegression, MeanFieldGuide, Trace_ELBO  # noqa: E402
from d3p_amd.svi import DPSVI  # noqa: E402


def create_toy_data(N, d, seed=123):
    """X ~ N(0, 1), y ~ Bernoulli(sigmoid(X w + b)) generated on the device (reference :88-104)."""
    lib = L.load()
    X = torch.empty((2 * N, d), dtype=torch.float32, device="cuda")
    y = torch.empty(2 * N, dtype=torch.float32, device="cuda")
    L.check(lib.d3p_synth_logreg(L.stream_ptr(), seed, 0, 2 * N, d, L.ptr(X), L.ptr(y)))
    return (X[:N].contiguous(), y[:N].contiguous()), (X[N:].contiguous(), y[N:].contiguous())


def estimate_accuracy(X, y, model, guide, params, rng, num_iterations=100):
    """Reference :110-116: the mean agreement of `num_iterations` posterior-predictive draws of the test labels with the labels."""
    from d3p_amd.modelling import sample_multi_posterior_predictive
    samples = sample_multi_posterior_predictive(rng, num_iterations, model, (X,), guide, (X,), params)
    return float((samples["obs"] == y.to(torch.int32)).float().mean())


def clipping_profile_report(svi, state, X, y):
    """The lines of --clipping-profile (d3p_amd.clipping): the quantiles of the per-example gradient norms of the whole table at the
    trained parameters, the share of rows the run's clipping threshold clips and the mean clip factor, and the median as the suggested
    threshold.  The numbers come from the private table without noise: they are a diagnostic, not a release."""
    from d3p_amd import clipping
    p = clipping.clipping_profile(svi, state, X, y)
    quant = ", ".join("{:g}% {:.4f}".format(100 * q, v) for q, v in zip(p.probs, p.quantiles))
    return ["clipping profile ({} rows, {} non-finite): gradient norm quantiles {}; mean {:.4f}, max {:.4f}".format(
                p.n, p.n_nonfinite, quant, p.mean, p.max),
            "at C = {:g}: clipped fraction {:.4f}, mean clip factor {:.4f}; suggested threshold (median norm) {:.4f}".format(
                p.thresholds[0], p.clipped_fraction[0], p.mean_clip_factor[0], clipping.suggest_clipping_threshold(p))]


def ppc_report(model, guide, params, X, y, num_draws, seed=7, statistics=("mean", "sd", "min", "max", "zeros")):
    """The lines of --ppc (d3p_amd.ppc): per statistic the observed value, the replicated mean and central 90 % range, p_ge and p_le
    of num_draws data sets replicated from the trained guide on the whole table."""
    from d3p_amd import ppc
    import d3p_amd.random.debug as jax_random
    res = ppc.posterior_predictive_check(jax_random.PRNGKey(seed), num_draws, model, (X, y), guide, params, statistics=statistics)
    return ["posterior predictive check ({} rows, {} replicated data sets):".format(res.n_rows, res.n_draws)] + res.lines()


def discrepancy_report(model, guide, params, X, y, num_draws, seed=8):
    """The lines of --discrepancy (d3p_amd.discrepancy): the paired p-values of the chi-square discrepancy, then mean and central 90 %
    range over num_draws draws from the trained guide of chi2_obs, chi2_rep, dispersion, both R^2 kinds, RMSE and bias."""
    from d3p_amd import discrepancy
    import d3p_amd.random.debug as jax_random
    res = discrepancy.discrepancy_check(jax_random.PRNGKey(seed), num_draws, model, (X, y), guide, params)
    return ["realized discrepancy check ({} rows, {} draws):".format(res.n_rows, res.n_draws)] + res.lines()


def classification_lines(model, guide, params, X, y, num_draws, seed=9, bins=10):
    """The lines of --classification-report (d3p_amd.classification): sampled accuracy +- sd with its 90 % interval over num_draws draws
    from the trained guide; accuracy, TPR, FPR and F1 at the threshold 0.5; auc [auc_lo, auc_hi], KS and ECE of the mean probability."""
    from d3p_amd import classification
    import d3p_amd.random.debug as jax_random
    return classification.classification_report(jax_random.PRNGKey(seed), num_draws, model, (X, y), guide, params, thresholds=(0.5,),
                                                bins=bins).lines()


def main(args):
    L.require_device()
    train, test = create_toy_data(args.num_samples, args.dimensions)
    N = args.num_samples
    q = args.batch_size / N
    train_init, train_fetch = poisson_batchify_data(train, q, max_batch_size=.99, rng_suite=rng_suite)
    test_init, test_fetch = split_batchify_data(test, batch_size=args.batch_size, rng_suite=rng_suite)

    dpsvi_rng = rng_suite.PRNGKey(0)
    dpsvi_rng, svi_init_rng, data_fetch_rng = rng_suite.split(dpsvi_rng, 3)
    num_iter_per_epoch, batchifier_state = train_init(rng_key=data_fetch_rng)
    sample_batch, _ = train_fetch(0, batchifier_state)

    dp_scale = getattr(args, "sigma", None)
    if dp_scale is None:  # examples/logistic_regression.py:135-137: calibrate the noise for the target epsilon
        from d3p_amd.dputil import approximate_sigma_remove_relation
        dp_scale, eps, _ = approximate_sigma_remove_relation(args.epsilon, delta=1 / N**2, q=q,
                                                             num_iter=num_iter_per_epoch * args.num_epochs)
        print("noise scale {:.4f} for epsilon {:.4f}, delta {:.2e}".format(dp_scale, eps, 1 / N**2))
    model = LogisticRegression(args.dimensions, prior_scale=1.0, intercept=True)
    guide = MeanFieldGuide(model) if getattr(args, "guide", "auto") == "handwritten" else AutoDiagonalNormal(model)
    svi = DPSVI(model, guide, Adam(args.learning_rate), Trace_ELBO(), dp_scale=dp_scale,
                clipping_threshold=1., num_obs_total=N, rng_suite=rng_suite)
    svi_state = svi.init(svi_init_rng, *sample_batch)

    accs, train_losses = [], []
    for i in range(args.num_epochs):
        t0 = time.time()
        dpsvi_rng, data_fetch_rng = rng_suite.split(dpsvi_rng, 2)
        num_batches, batchifier_state = train_init(rng_key=data_fetch_rng)
        svi_state, losses = svi.run_steps(svi_state, train_fetch, batchifier_state, 0, num_batches)
        train_loss = float(losses.sum()) / (N * num_batches)
        torch.cuda.synchronize()
        t1 = time.time()

        dpsvi_rng, test_fetch_rng = rng_suite.split(dpsvi_rng, 2)
        num_test_batches, test_state = test_init(rng_key=test_fetch_rng)
        params = svi.get_params(svi_state)
        if "w_loc" in params:   # the hand-written guide's leaves
            w, b = params["w_loc"], params["intercept_loc"]
        else:
            w, b = params["auto_loc"][:-1], params["auto_loc"][-1]
        test_loss, acc = 0.0, 0.0
        for j in range(num_test_batches):
            bx, by = test_fetch(j, test_state)
            test_loss += float(svi.evaluate(svi_state, bx, by)) / (N * num_test_batches)
            acc += float(((bx @ w + b > 0).float() == by).float().mean()) / num_test_batches
        accs.append(acc)
        train_losses.append(train_loss)
        print("Epoch {}: loss = {:.4f}, acc = {:.4f} (loss on training set: {:.4f}) ({:.3f} s.)".format(
            i, test_loss, acc, train_loss, t1 - t0))
    if getattr(args, "predictive_accuracy", False):   # reference :230 (its posterior half)
        import d3p_amd.random.debug as jax_random
        acc_post = estimate_accuracy(test[0], test[1], model, guide, svi.get_params(svi_state), jax_random.PRNGKey(1), 100)
        print("avg accuracy on test set with found posterior (100 posterior-predictive draws): {:.4f}".format(acc_post))
        from d3p_amd.predictive import posterior_predictive_samples   # the regression family's sampler: modelling's draws for this model
        pred = posterior_predictive_samples(jax_random.PRNGKey(1), 100, model, (test[0],), guide, svi.get_params(svi_state))["obs"]
        print("posterior predictive check (100 draws): observed mean {:.4f}, predictive mean {:.4f}".format(
            float(test[1].mean()), float(pred.float().mean())))
    if getattr(args, "clipping_profile", False):   # both guides: the hand-written one draws its eps per site
        print("\n".join(clipping_profile_report(svi, svi_state, *train)))
    if getattr(args, "ppc", None) is not None:   # both guides
        print("\n".join(ppc_report(model, guide, svi.get_params(svi_state), *train, args.ppc)))
    if getattr(args, "discrepancy", None) is not None:   # both guides
        print("\n".join(discrepancy_report(model, guide, svi.get_params(svi_state), *train, args.discrepancy)))
    if getattr(args, "classification_report", None) is not None:
        if isinstance(guide, MeanFieldGuide):
            print("classification report: --guide auto only (d3p_amd.classification runs AutoDiagonalNormal and DiagonalNormalGuide)")
        else:
            print("\n".join(classification_lines(model, guide, svi.get_params(svi_state), *test, args.classification_report)))
    return accs, train_losses


if __name__ == "__main__":
    parser = argparse.ArgumentParser(description="parse args")
    parser.add_argument('-e', '--epsilon', default=.1, type=float, help='privacy epsilon (delta = 1 / N^2)')
    parser.add_argument('--sigma', default=None, type=float, help='dp_scale of the Gaussian mechanism (overrides --epsilon)')
    parser.add_argument('-n', '--num-epochs', default=10, type=int, help='number of training epochs')
    parser.add_argument('-lr', '--learning-rate', default=1.0e-2, type=float, help='learning rate')
    parser.add_argument('-batch-size', default=200, type=int, help='batch size')
    parser.add_argument('-d', '--dimensions', default=4, type=int, help='data dimension')
    parser.add_argument('-N', '--num-samples', default=10000, type=int, help='data samples count')
    parser.add_argument('--guide', choices=["auto", "handwritten"], default="auto",
                        help="auto: AutoDiagonalNormal (README.md:99); handwritten: the reference script's own two-site guide (:67-86)")
    parser.add_argument('--predictive-accuracy', action='store_true',
                        help="after training, print the test accuracy of 100 posterior-predictive draws (reference :110-116, :230)")
    parser.add_argument('--clipping-profile', action='store_true',
                        help='after training, report the quantiles of the per-example gradient norms on the whole table, the share of '
                             'rows the clipping threshold clips and the suggested threshold (a diagnostic of the private table, not a release)')
    parser.add_argument('--ppc', nargs='?', const=100, default=None, type=int, metavar='N_DRAWS',
                        help='after training, print the posterior predictive check of N_DRAWS (default 100) replicated data sets: per '
                             'statistic the observed value, the replicated mean and 90 %% range, p_ge and p_le')
    parser.add_argument('--discrepancy', nargs='?', const=100, default=None, type=int, metavar='N_DRAWS',
                        help='after training, print the chi-square realized-discrepancy check of N_DRAWS (default 100) draws: p_ge, p_le, '
                             'the dispersion, the Bayesian R^2, RMSE and bias per draw')
    parser.add_argument('--classification-report', nargs='?', const=100, default=None, type=int, metavar='N_DRAWS',
                        help='after training, print on the test table the sampled accuracy of N_DRAWS (default 100) posterior draws with '
                             'its sd, accuracy / TPR / FPR / F1 at 0.5, and the AUC with its certificate, KS and ECE of the mean probability')
    main(parser.parse_args())
