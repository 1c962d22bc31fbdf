"""Priors on the hot path: fast_gp (GP, RBF), fast_gp_mix (Matern-5/2 ARD with Gamma hyper-priors), mlp (BNN prior), stroke (the few-shot study's glyphs), omniglot (its episode loader over an image bank on the device), with prior / utils plumbing;
plus the two cheap priors of SURVEY.md 8(f) row 4 (ridge, binarized_regression) and the prior from a user-defined generative model (pyro: the name is the
reference's, the module is plain torch).  Unlike the reference package (priors/__init__.py:1) nothing here depends on gpytorch / botorch / pyro."""
from transformerscandobayesianinference_amd.priors import prior, utils, fast_gp, fast_gp_mix, mlp, ridge, binarized_regression, pyro, stroke, omniglot  # noqa: F401
