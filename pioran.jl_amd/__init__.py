"""pioran.jl_amd — MI355X-native ScalableGP log-likelihood hot path (drop-in for that path of Pioran.jl).

Directory name has a dot, so import it through the repo-root shim: `import pioran_jl_amd as pj`.
"""
from . import _lib, farm  # noqa: F401
from .gp import (Context, CustomMean, Dataset, Farm, FiniteScalableGP, PosteriorGP, ScalableGP, cov, default_context,
                 log_likelihood, log_likelihood_direct, logl, logpdf, logpdf_batch, lombscargle, lsp_ppc, lsp_ppc_frequencies, mean, posterior, ppc_t_pred, ppc_timeseries, ppc_timeseries_summary, predict, predict_cov, predict_direct,
                 predict_var, quantiles, rand, rand_posterior, simulate, std, var)
from .gp import posterior_predict_checks, psd_ppc, psd_ppc_carma, run_diagnostics, sample_approx_model
from .carma import (CARMA_normalisation, check_conjugate_pair, check_order_imag_roots, check_roots_bounds, evaluate, quad2roots, roots2coeffs,
                    sample_quad)
from .kernels import (CARMA, Celerite, Exp, ScaledKernel, SemiSeparable, SHO, SumOfCelerite, SumOfSemiSeparable,
                      SumOfTerms, celerite_coefs)
from .psd import (QPO, DoubleBendingPowerLaw, SingleBendingPowerLaw, approx, approx_batch, approx_batch_qpo, approx_batch_qpo_vjp, approx_batch_vjp, approximated_psd,
                  build_approx, convert_feature, get_approx_coefficients, get_norm_psd, psd_decomp, separate_psd)

__all__ = [n for n in dir() if not n.startswith("_")]
