"""Prior from a user-defined generative model (reference priors/pyro.py:10-34): `config['model']` is any callable that returns an object with
`__call__(seq_len=) -> (x [T,F], y [T])` -- in the reference a PyroModule, here anything (mcmc_svi_transformer_on_bayesian.BayesianModel is one), so
nothing depends on pyro.  The draws are whatever the model does; the transformer they feed runs through the HIP stack like every other prior's.
"""
import torch

from transformerscandobayesianinference_amd.priors.utils import get_batch_to_dataloader


def get_batch(batch_size, seq_len, batch_size_per_gp_sample=None, **config):
    """`batch_size // batch_size_per_gp_sample` models (default: 16 datasets per model), `batch_size_per_gp_sample` datasets from each; x is
    standardised over the sequence axis, (x - mean) / (std + 1e-6).  Returns (x [T,B,F], y [T,B], y); keys of `config` other than 'model' are ignored."""
    batch_size_per_gp_sample = batch_size_per_gp_sample or batch_size // 16
    assert batch_size_per_gp_sample and batch_size % batch_size_per_gp_sample == 0, 'Please choose a batch_size divisible by batch_size_per_gp_sample.'
    num_models = batch_size // batch_size_per_gp_sample
    models = [config['model']() for _ in range(num_models)]
    sample = [model(seq_len=seq_len) for model in models for _ in range(batch_size_per_gp_sample)]
    x, y = zip(*sample)
    y = torch.stack(y, 1).squeeze(-1).detach()
    x = torch.stack(x, 1).detach()
    x = (x - x.mean(0)) / (x.std(0) + .000001)
    return x, y, y


DataLoader = get_batch_to_dataloader(get_batch)
DataLoader.num_outputs = 1
