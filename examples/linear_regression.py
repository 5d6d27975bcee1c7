#!/usr/bin/env python3
"""Bayesian linear regression with DP-VI on MI355X: toy data generated on the device, the declared model LinearRegression
with AutoDiagonalNormal, training with the device-resident loop (`run_steps`), then the loss and the distance of the posterior mean
from the weights that generated the data.

    w ~ Normal(0, 1)^d, intercept ~ Normal(0, 1);  ys ~ Normal(xs @ w + intercept, obs_scale)

--guide-diagnostic [N_DRAWS] (off by default; d3p_amd.diagnostics) adds one line after training: the full-data ELBO +- its standard
error, the importance-sampling estimate of the log evidence, the Pareto k of the guide's importance ratios against its threshold and
their effective sample size (Yao et al. 2018: is the trained guide a usable approximation of the posterior?).

--intervals [N_DRAWS] (off by default; d3p_amd.intervals) adds, after training: the share of the observed outcomes inside the
equal-tailed 90 % posterior predictive interval of N_DRAWS draws, the interval's mean width, and mean, std, median and the 5 % / 95 %
quantiles of the draws of every weight.
--interval-kind {equal-tailed,hpdi} (default equal-tailed; read only with --intervals): with hpdi the coverage and width lines are those
of the 90 % highest-density interval (numpyro's hpdi, kind="hpdi") and the summary of `w` reports that interval's ends
(latent_summary(interval="hpdi")), as numpyro's print_summary does; the lines say which kind they are.

--clipping-profile (off by default; d3p_amd.clipping) adds two lines after training: the quantiles of the per-example gradient norms of
the whole table at the trained parameters, the share of rows the run's clipping threshold clips with the mean clip factor, and the
median norm as the suggested threshold (Abadi et al. 2016).  They are computed from the private table without noise.
--crps [N_DRAWS] (off by default; d3p_amd.scoring) adds, after training, on a held-out test split -- 2000 fresh rows from the process
that generated the training table -- three lines: the mean CRPS of N_DRAWS posterior predictive draws against the observed outcomes +- its
standard error, with its two parts (mae = E|X - y|, spread = 1/2 E|X - X'|); and the ten-bin PIT histogram as a density (1 in every bin:
calibrated; a U shape: the predictive is too narrow; a hump: too wide).
--ppc [N_DRAWS] (off by default; d3p_amd.ppc) adds, after training, one line per statistic -- mean, sd, min, max, zeros -- of the
posterior predictive check on the training table: the statistic of the observed outcomes, its mean and central 90 % range over N_DRAWS
data sets replicated from the trained guide, and the tail shares p_ge = P(T(y_rep) >= T(y)) and p_le.  The replicated data sets are
reduced as they are drawn; they are never written.
--discrepancy [N_DRAWS] (off by default; d3p_amd.discrepancy) adds, after training, the realized-discrepancy check of Gelman, Meng &
Stern (1996) on the training table: per draw from the trained guide the Pearson chi-square of the observed outcomes and of that draw's
own replicate, the share p_ge of draws whose replicate is at least as far from the mean as the data, the dispersion chi2_obs / rows
(near 1 where --obs-scale is the noise of the data), and the Bayesian R^2 (both kinds), RMSE and bias per draw.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import d3p_amd._lib as L  # noqa: E402
import d3p_amd.random as rng_suite  # noqa: E402
from d3p_amd.minibatch import subsample_batchify_data  # noqa: E402
from d3p_amd.models import Adam, AutoDiagonalNormal, LinearRegression, Trace_ELBO  # noqa: E402
from d3p_amd.svi import DPSVI  # noqa: E402


def create_toy_data(N, d, seed=123, obs_scale=0.5):
    """w_true ~ N(0, 1 / d), X ~ N(0, 1), y = X w_true + obs_scale * N(0, 1), on the device with a fixed seed."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    w_true = torch.randn(d, generator=g, device="cuda") / d ** 0.5
    X = torch.randn(N, d, generator=g, device="cuda")
    y = X @ w_true + obs_scale * torch.randn(N, generator=g, device="cuda")
    return X.contiguous(), y.to(torch.float32).contiguous(), w_true


def guide_diagnostic_report(model, svi, state, X, y, num_draws, seed=3):
    """The guide diagnostic line (d3p_amd.diagnostics): ELBO, importance-sampling evidence, Pareto k and effective sample size of
    num_draws draws from the trained guide on the whole table."""
    from d3p_amd import diagnostics
    import d3p_amd.random.debug as jax_random
    res = diagnostics.guide_diagnostic(jax_random.PRNGKey(seed), num_draws, model, (X, y), svi.guide, svi.get_params(state))
    return ("guide diagnostic ({} rows, {} draws): elbo {:.2f} +- {:.2f}, log_evidence_is {:.2f}, pareto k {:.2f} (threshold {:.2f}), "
            "ess {:.1f}").format(res.n_rows, res.n_draws, float(res.elbo), float(res.elbo_se), float(res.log_evidence_is),
                                 float(res.pareto_k), res.k_threshold, float(res.ess))


def intervals_report(model, svi, state, X, y, num_draws, seed=4, kind="equal_tailed"):
    """The lines of --intervals (d3p_amd.intervals): the share of the observed y inside the equal-tailed 90 % posterior predictive
    interval of num_draws draws from the trained guide, the interval's mean width, and the summary of the draws of `w`.
    kind="hpdi" (--interval-kind hpdi): the same of the highest-density interval, and the lines say so."""
    from d3p_amd import intervals
    from d3p_amd.predictive import posterior_predictive_samples
    import d3p_amd.random.debug as jax_random
    key, params = jax_random.PRNGKey(seed), svi.get_params(state)
    hp = kind == "hpdi"
    iv = intervals.posterior_predictive_interval(key, num_draws, model, (X,), svi.guide, params, prob=0.9, **({"kind": "hpdi"} if hp else {}))
    inside = ((y >= iv["lower"]) & (y <= iv["upper"])).double().mean()
    width = (iv["upper"].double() - iv["lower"].double()).mean()
    lines = ["90% {}predictive interval ({} rows, {} draws): coverage {:.4f}, mean width {:.4f}".format(
        "highest-density " if hp else "", X.shape[0], num_draws, float(inside), float(width))]
    draws = posterior_predictive_samples(key, num_draws, model, (X[:1],), svi.guide, params)   # (the same latents: they take no row)
    s = {k: v.double().cpu() for k, v in intervals.latent_summary({"w": draws["w"]}, prob=0.9, **({"interval": "hpdi"} if hp else {}))["w"].items()}
    ends = "90% hpdi {:.4f} .. {:.4f}" if hp else "5% {:.4f}, 95% {:.4f}"
    for j in range(s["mean"].shape[0]):
        lines.append(("w[{}]: mean {:.4f}, std {:.4f}, median {:.4f}, " + ends).format(
            j, float(s["mean"][j]), float(s["std"][j]), float(s["median"][j]), float(s["lower"][j]), float(s["upper"][j])))
    return lines


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


def create_test_data(w_true, rows, obs_scale, seed=321):
    """The held-out test split of --crps: fresh rows from the process of create_toy_data at the same w_true, on a seed of their own."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    X = torch.randn(rows, w_true.shape[0], generator=g, device="cuda")
    y = X @ w_true + obs_scale * torch.randn(rows, generator=g, device="cuda")
    return X.contiguous(), y.to(torch.float32).contiguous()


def crps_report(model, svi, state, X_test, y_test, num_draws, seed=5):
    """The lines of --crps (d3p_amd.scoring): mean CRPS +- its standard error with mae and spread, and the ten-bin PIT histogram as a
    density, of num_draws posterior predictive draws against the test split's observed outcomes."""
    from d3p_amd import scoring
    import d3p_amd.random.debug as jax_random
    res = scoring.posterior_predictive_crps(jax_random.PRNGKey(seed), num_draws, model, (X_test, y_test), svi.guide, svi.get_params(state))
    density = (res.pit_histogram / res.n_rows * res.pit_histogram.shape[0]).cpu().tolist()
    return ["CRPS on the test split ({} rows, {} draws): {:.4f} +- {:.4f}".format(res.n_rows, res.n_draws, float(res.crps), float(res.se)),
            "mae {:.4f}, spread {:.4f}".format(float(res.mae), float(res.spread)),
            "PIT histogram (density, 10 bins): " + " ".join("{:.3f}".format(v) for v in density)]


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


def main(args):
    L.require_device()
    N, d = args.num_samples, args.dimensions
    X, y, w_true = create_toy_data(N, d, obs_scale=args.obs_scale)
    model = LinearRegression(d, prior_scale=1.0, intercept=True, obs_scale=args.obs_scale)
    svi = DPSVI(model, AutoDiagonalNormal(model), Adam(args.learning_rate), Trace_ELBO(), dp_scale=args.sigma,
                clipping_threshold=args.clip_threshold, num_obs_total=N, rng_suite=rng_suite)
    key, init_key, batch_key = rng_suite.split(rng_suite.PRNGKey(0), 3)
    init, get_batch = subsample_batchify_data((X, y), args.batch_size, rng_suite=rng_suite)
    _, batchifier_state = init(rng_key=batch_key)
    state = svi.init(init_key, *get_batch(0, batchifier_state))
    err0 = float((svi.get_params(state)["auto_loc"][:d] - w_true).norm())
    state, losses = svi.run_steps(state, get_batch, batchifier_state, 0, args.num_steps)
    torch.cuda.synchronize()
    k = max(1, args.num_steps // 10)
    first, last = float(losses[:k].mean()) / N, float(losses[-k:].mean()) / N
    err = float((svi.get_params(state)["auto_loc"][:d] - w_true).norm())
    print("loss per example: first {:.4f} -> last {:.4f};  |loc - w_true|: {:.4f} -> {:.4f}".format(first, last, err0, err))
    # posterior predictive check: the observed outcomes against 100 draws of `obs` at the trained parameters
    from d3p_amd.predictive import posterior_predictive_samples
    import d3p_amd.random.debug as jax_random
    pred = posterior_predictive_samples(jax_random.PRNGKey(1), 100, model, (X,), svi.guide, svi.get_params(state))["obs"].double()
    print("posterior predictive check (100 draws): observed mean {:.4f}, variance {:.4f};  predictive mean {:.4f}, variance {:.4f}".format(
        float(y.mean()), float(y.var()), float(pred.mean()), float(pred.var(dim=1).mean())))
    if getattr(args, "guide_diagnostic", None) is not None:
        print(guide_diagnostic_report(model, svi, state, X, y, args.guide_diagnostic))
    if getattr(args, "intervals", None) is not None:
        kind = (getattr(args, "interval_kind", None) or "equal-tailed").replace("-", "_")
        print("\n".join(intervals_report(model, svi, state, X, y, args.intervals, kind=kind)))
    if getattr(args, "clipping_profile", False):
        print("\n".join(clipping_profile_report(svi, state, X, y)))
    if getattr(args, "crps", None) is not None:
        X_test, y_test = create_test_data(w_true, 2000, args.obs_scale)
        print("\n".join(crps_report(model, svi, state, X_test, y_test, args.crps)))
    if getattr(args, "ppc", None) is not None:
        print("\n".join(ppc_report(model, svi.guide, svi.get_params(state), X, y, args.ppc)))
    if getattr(args, "discrepancy", None) is not None:
        print("\n".join(discrepancy_report(model, svi.guide, svi.get_params(state), X, y, args.discrepancy)))
    return first, last, err0, err


if __name__ == "__main__":
    parser = argparse.ArgumentParser(description="parse args")
    parser.add_argument('--sigma', default=0.5, type=float, help='dp_scale of the Gaussian mechanism')
    parser.add_argument('--clip-threshold', default=1.0, type=float, help='clipping threshold of the per-example gradients')
    parser.add_argument('-n', '--num-steps', default=2000, type=int, help='number of training steps')
    parser.add_argument('-lr', '--learning-rate', default=2.0e-2, type=float, help='learning rate')
    parser.add_argument('-batch-size', default=200, type=int, help='batch size')
    parser.add_argument('-d', '--dimensions', default=4, type=int, help='data dimension')
    parser.add_argument('-N', '--num-samples', default=10000, type=int, help='data samples count')
    parser.add_argument('--obs-scale', default=0.5, type=float, help='standard deviation of the observation noise')
    parser.add_argument('--guide-diagnostic', nargs='?', const=100, default=None, type=int, metavar='N_DRAWS',
                        help='after training, report the ELBO, the importance-sampling evidence, the Pareto k and the effective sample '
                             'size of N_DRAWS (default 100) draws from the guide on the whole table')
    parser.add_argument('--intervals', nargs='?', const=100, default=None, type=int, metavar='N_DRAWS',
                        help='after training, report the coverage and the mean width of the 90 %% posterior predictive interval of '
                             'N_DRAWS (default 100) draws on the whole table, and the summary of the draws of w')
    parser.add_argument('--interval-kind', choices=('equal-tailed', 'hpdi'), default='equal-tailed',
                        help='with --intervals: the equal-tailed interval (quantiles) or the highest-density interval (numpyro hpdi)')
    parser.add_argument('--clipping-profile', action='store_true',
                        help='after training, report the quantiles of the per-example gradient norms on the whole table, the share of '
                             'rows the clipping threshold clips and the suggested threshold (a diagnostic of the private table, not a release)')
    parser.add_argument('--crps', nargs='?', const=100, default=None, type=int, metavar='N_DRAWS',
                        help='after training, report the mean CRPS with mae and spread and the PIT histogram of N_DRAWS (default 100) '
                             'posterior predictive draws on a held-out test split')
    parser.add_argument('--ppc', nargs='?', const=100, default=None, type=int, metavar='N_DRAWS',
                        help='after training, print the posterior predictive check of N_DRAWS (default 100) replicated data sets: per '
                             'statistic the observed value, the replicated mean and 90 %% range, p_ge and p_le')
    parser.add_argument('--discrepancy', nargs='?', const=100, default=None, type=int, metavar='N_DRAWS',
                        help='after training, print the chi-square realized-discrepancy check of N_DRAWS (default 100) draws: p_ge, p_le, '
                             'the dispersion, the Bayesian R^2, RMSE and bias per draw')
    main(parser.parse_args())
