"""Tabular entry point: build (and optionally train) the PFN that `TabularEvalSimple.ipynb` evaluates, and the
checkpoint convention the notebooks use to hand a trained model around.

Mirror of the model-building part of the reference `tabular.py`:
    get_uniform_single_eval_pos_sampler   :39-44
    get_*_prior_hyperparameters           :47-106
    get_model                             :109-155
plus `save_checkpoint` / `load_checkpoint` for the `(state_dict, optimizer_state)` tuples of
`BayesianModels_And_Custom_Pyro_Modules.ipynb` cells 14 / 16 and `TabularEvalSimple.ipynb` cell 12.

The evaluation protocol of the reference file runs on the device:
    evaluate / evaluate_dataset / evaluate_position / batch_pred     :160-323
    knn_metric (with its 5-fold grid search over k)                  :350-369
    load_svmlight_table                                              datasets/__init__.py:8-16
`evaluate_position` gathers and normalises every (window, test row) column in one launch (pfn_tabular_windows), runs the PFN once
at batch windows x test rows, and counts ROC-AUC pairs on the device (pfn_auc_counts); the kNN baseline finds the neighbour lists of
every CV fold and every test row of every window in one launch (pfn_knn_cv) and does the grid-search arithmetic on the host in f64.
    logistic_metric (with its grid search over 108 parameter sets)   :325-346
solves every candidate and fold of every window to its optimum in one launch (pfn_logistic_cv); the grid, the folds and the scores are host
arithmetic in f64.
    gp_metric (with its grid search over 24 kernels c * RBF(l))      :480-503
restates scikit-learn's binary Laplace GaussianProcessClassifier: pfn_gpc_lml_grad gives the log marginal likelihood and its gradient of every candidate and fold
of every window in one launch per L-BFGS pass (`priors.fast_gp_mix.batched_lbfgs` on the host drives it), pfn_gpc_predict the decision values and variances
(DESIGN.md 21); folds, scores, selection and the erf-mixture probabilities are host arithmetic in f64.  It needs no library beyond this stack.
    bayes_net_metric (with its grid search over 8 (width, lr) pairs) :372-478
runs the 400 SVI steps and the 400 predictive draws of every candidate and fold of every window in one launch (pfn_bnn_cv): the model, the guide
and the step are those of the BNN study's `eval_svi`; the folds, the starts, the scores and the selection are host arithmetic.  The reference's own grid search
raises on two keys of param_grid['bayes'] that are no constructor arguments; what it evidently means is built here.
    xgb_metric (with its grid search over 16 boosting parameter sets) :599-626
restates the exact greedy algorithm of gradient-boosted trees on logistic loss (depth 1 or 2, 100 rounds, row and column sampling from Philox) and runs every
round of every candidate and fold of every window in one launch (pfn_xgb_cv); the grid, the 5 folds, the scores and the selection are host
arithmetic in f64.  No boosting library is carried, so nothing is pinned to one: include/pfn_hip.h is the specification.
    catboost_metric (with its grid search over 81 parameter sets)    :556-596
restates CatBoost's symmetric trees on logistic loss (Cosine score with its random strength, Newton leaf values with backtracking, depth 2, 4 or 7) and grows
every tree of every distinct fit of every window in one launch (pfn_catboost_cv): 'iterations' only cuts a fit short, so the 81 entries are 27
fits read at three checkpoints.  The grid, the stratified 80/20 hold-out that the library's grid_search scores the entries on, the log losses and the selection
are host arithmetic in f64; everything about the library is restated from memory and pinned to nothing.
The OpenML loaders stay out: they need libraries and network access this stack
does not carry.  Any callable with the reference's metric-function
signature still runs through `batch_pred`, one window at a time, as the reference loops.

`get_model` trains through this package's `train()` -- HIP encoder stack, fused optimizer, HIP prior samplers --
so a PFN trained here loads into the reference's `TransformerModel` and vice versa: the state-dict keys are the
reference's.
"""
import functools
import os
import time
import warnings

import numpy as np
import torch
from torch import nn

from transformerscandobayesianinference_amd import encoders, hipops, priors
from transformerscandobayesianinference_amd.priors.utils import gamma_sampler_f, trunc_norm_sampler_f
from transformerscandobayesianinference_amd.train import Losses, train
from transformerscandobayesianinference_amd.utils import get_uniform_single_eval_pos_sampler  # noqa: F401  (reference tabular.py:39-44 defines it here)


def _only(named_sampler: dict):
    """The notebook configs wrap every sampler as {'description': callable}; the callable is what the prior wants."""
    return next(iter(named_sampler.values()))


def get_mlp_prior_hyperparameters(config):
    """The 17-tuple `priors.mlp.get_batch` unpacks (priors/mlp.py:103-112), from a notebook config dict
    (`TabularEvalSimple.ipynb` cell 7).  The causal-graph fields are only filled when `prior_is_causal`."""
    causal = config['prior_is_causal']
    when_causal = lambda value: value if causal else None
    return (
        _only(config['prior_nlayers_sampler']),
        _only(config['prior_emsize_sampler']),
        config['prior_activations'],
        gamma_sampler_f(config['prior_sigma_gamma_k'], config['prior_sigma_gamma_theta']),          # init / weight std
        gamma_sampler_f(config['prior_noise_std_gamma_k'], config['prior_noise_std_gamma_theta']),  # per-layer noise std
        _only(config['prior_dropout_sampler']),
        True,                                                                                        # binary labels
        _only(config['prior_num_features_used_sampler']),
        _only(config['prior_causes_sampler']) if causal else None,
        causal,
        when_causal(config.get('prior_pre_sample_causes')),
        when_causal(config.get('prior_pre_sample_weights')),
        when_causal(config.get('prior_y_is_effect')),
        config['prior_order_y'],
        config['prior_normalize_by_used_features'],
        _only(config['prior_categorical_feats']) if causal else None,
        0.0,                                                                                         # nan_prob
    )


def get_gp_mix_prior_hyperparameters(config):
    """Hyper-prior dict of `priors.fast_gp_mix`.  Reference quirk kept on purpose (tabular.py:72-79): the two keys
    'categorical_data' and 'y_minmax_norm' are fed from `prior_y_minmax_norm` and `prior_lengthscale_concentration`
    respectively, so `y_minmax_norm` ends up truthy whenever the lengthscale concentration is non-zero."""
    return {
        'lengthscale_concentration': config['prior_lengthscale_concentration'],
        'nu': config['prior_nu'],
        'outputscale_concentration': config['prior_outputscale_concentration'],
        'categorical_data': config['prior_y_minmax_norm'],
        'y_minmax_norm': config['prior_lengthscale_concentration'],
        'noise_concentration': config['prior_noise_concentration'],
        'noise_rate': config['prior_noise_rate'],
    }


def get_gp_prior_hyperparameters(config):
    """7-tuple of the reference's 'gp' prior type (tabular.py:82-91): constant outputscale / lengthscale wrapped as samplers."""
    outputscale, lengthscale = config['prior_outputscale'], config['prior_lengthscale']
    return (config['prior_noise'], lambda: outputscale, lambda: lengthscale, True,
            _only(config['prior_num_features_used_sampler']), config['prior_normalize_by_used_features'], config['prior_order_y'])


def get_meta_gp_prior_hyperparameters(config):
    """7-tuple of the 'custom_gp_mix' prior type (tabular.py:94-105): truncated-normal samplers around the configured means."""
    def around(mean_key, std_factor_key):
        return trunc_norm_sampler_f(config[mean_key], config[mean_key] * config[std_factor_key])
    return (config['prior_noise'], around('prior_outputscale_mean', 'prior_outputscale_std_f'),
            around('prior_lengthscale_mean', 'prior_lengthscale_std_f'), True,
            _only(config['prior_num_features_used_sampler']), config['prior_normalize_by_used_features'], config['prior_order_y'])


def _prior_for(config):
    kind = config['prior_type']
    if kind == 'mlp':
        return priors.mlp.DataLoader, get_mlp_prior_hyperparameters(config), {'batch_size_per_gp_sample': 8}
    if kind == 'gp_mix':
        return priors.fast_gp_mix.DataLoader, get_gp_mix_prior_hyperparameters(config), {}
    if kind in ('gp', 'custom_gp_mix'):
        # the reference hands these 7-tuples (with callables for outputscale / lengthscale) to priors.fast_gp.get_batch,
        # which reads entries 0..2 as plain GP hyper-parameters -- that path cannot run there either (the notebook
        # raises "Not Implemented" for it, TabularEvalSimple.ipynb cell 12).  Draw the constants once instead.
        hps = get_gp_prior_hyperparameters(config) if kind == 'gp' else get_meta_gp_prior_hyperparameters(config)
        return priors.fast_gp.DataLoader, (hps[0], float(hps[1]()), float(hps[2]())), {}
    raise ValueError(f"unknown prior_type {kind!r} (mlp, gp, custom_gp_mix, gp_mix)")


def get_model(config, device, eval_positions, should_train=True, verbose=False, **train_kwargs):
    """Reference tabular.py:109-155: a binary-classification PFN (`Losses.bce`, one output) for the prior named by
    `config['prior_type']`; `should_train=False` only builds it (0 epochs) so a checkpoint can be loaded into it.
    Returns train()'s 3-tuple; the notebooks take element [2], the model.  `train_kwargs` reach `train()`
    (e.g. steps_per_epoch, precision) -- the reference fixes steps_per_epoch at 100."""
    prior_class, hyperparameters, extra = _prior_for(config)
    epochs = config['epochs'] if should_train else 0
    kwargs = dict(steps_per_epoch=100)
    kwargs.update(train_kwargs)
    return train(prior_class, Losses.bce, encoders.Linear,
                 emsize=config['emsize'], nhead=config['nhead'], nhid=config['emsize'] * config['nhid_factor'],
                 nlayers=config['nlayers'], dropout=config['dropout'], y_encoder_generator=encoders.Linear,
                 pos_encoder_generator=None, batch_size=config['batch_size'], bptt=config['bptt'], lr=config['lr'],
                 epochs=epochs, warmup_epochs=epochs // 4, gpu_device=device, verbose=verbose,
                 single_eval_pos_gen=get_uniform_single_eval_pos_sampler(max(eval_positions) + 1),
                 extra_prior_kwargs_dict={'num_features': config['num_features'], 'fuse_x_y': False,
                                          'hyperparameters': hyperparameters, 'device': device, **extra},
                 **kwargs)


def save_checkpoint(model, path, optimizer_state=None):
    """`torch.save((state_dict, optimizer_state), path)` -- the tuple the notebooks write and read."""
    state = {k: v.detach().to('cpu') for k, v in model.state_dict().items()}
    torch.save((state, optimizer_state), path)


def load_checkpoint(model, path, strict=True):
    """Inverse of `save_checkpoint`; also reads checkpoints written by the reference.  Returns the optimizer state
    stored next to the weights (None in every checkpoint the reference ships)."""
    model_state, optimizer_state = torch.load(path, map_location='cpu')
    model.load_state_dict(model_state, strict=strict)
    return optimizer_state


## General eval (reference tabular.py:158-323)

CV = 5                      # the reference's module constant: folds of every grid search
MAX_TOKENS_PER_FORWARD = 1 << 20


def load_svmlight_table(path):
    """The class-balancing, interleaving loader of the reference's datasets/__init__.py:8-16 (`get_svmlight`) for a local svmlight / libsvm text file with
    labels -1 / +1: keep all rows of the rarer class and as many of the other (the LAST ones in file order), alternate the two classes, reverse.  Returns
    (X [2 m, F] f32, y [2 m] f32 in {0, 1}).  Rows of equal label keep their file order (a stable sort; the reference's `np.argsort` default is not stable, so
    its order there depends on the numpy build -- INTEGRATION.md)."""
    labels, rows, width = [], [], 0
    with open(path) as f:
        for line in f:
            line = line.split('#', 1)[0].split()
            if not line:
                continue
            labels.append(float(line[0]))
            pairs = [(int(k), float(v)) for k, v in (item.split(':') for item in line[1:] if not item.startswith('qid:'))]
            rows.append(pairs)
            width = max([width] + [k for k, _ in pairs])
    one_based = all(k >= 1 for pairs in rows for k, _ in pairs)      # sklearn's zero_based='auto'
    width = width if one_based else width + 1
    X = np.zeros((len(rows), width), dtype=np.float64)
    for i, pairs in enumerate(rows):
        for k, v in pairs:
            X[i, k - 1 if one_based else k] = v
    y = (np.asarray(labels, dtype=np.float64) + 1) / 2
    minority_is_one = y.mean() < 0.5
    order = np.argsort(y if minority_is_one else -y, kind='stable')
    m = int(y.sum()) if minority_is_one else int((1 - y).sum())
    X, y = X[order][-2 * m:], y[order][-2 * m:]
    y = torch.tensor(y).reshape(2, -1).transpose(0, 1).reshape(-1).flip([0]).float()
    X = torch.tensor(X).reshape(2, -1, X.shape[1]).transpose(0, 1).reshape(-1, X.shape[1]).flip([0]).float()
    return X, y


def roc_auc_columns(scores, labels):
    """ROC-AUC of every column of scores [T, C] against labels [T, C] in {0, 1} (both on the GPU): the device counts pairs (pfn_auc_counts), the host forms
    (2 gt + eq) / (2 P Nn) in f64 -- sklearn's `roc_auc_score` as a ratio of integers.  Returns (auc [C] numpy f64, columns left NaN because they hold one
    class only; the reference raises there)."""
    auc = hipops.auc_from_counts(hipops.auc_counts(scores.float().contiguous(), labels.float().contiguous()))
    return auc, int(np.isnan(auc).sum())


def _report_undefined(undefined, what):
    if undefined:
        warnings.warn(f'{undefined} {what} hold one class only: their ROC-AUC is NaN')


def evaluate(datasets, model, method, bptt, eval_position_range, device, max_features=0, plot=False, extend_features=False, save=True, rescale_features=False,
             overwrite=False, max_samples=40, path_interfix='', save_dir=None):
    """Reference tabular.py:160-213: `datasets` = [[name, X, y, categorical_feats], ...]; `model` a PFN (nn.Module) or a metric function of this module (or
    any callable with that signature); returns the reference's result dict.  The reference's hard-coded results folder is `save_dir`: with None nothing is read
    or written; otherwise a dataset's results are loaded from `{save_dir}/{path_interfix}/results_{method}_{name}.npy` when that file exists (and not
    `overwrite`), and written there when `save`.  `plot` is accepted and ignored.  `extend_features` pads the table to `max_features` columns of zeros inside
    the window kernel (no padded copy of the table is made); `rescale_features` divides by num_features / max_features as the reference does."""
    result = {'metric': 'auc'}
    eval_position_range = list(eval_position_range)
    for [name, X, y, categorical_feats] in datasets:
        result_ds = {}
        path = None if save_dir is None else os.path.join(str(save_dir), path_interfix, f'results_{method}_{name}.npy')
        if path is not None and os.path.isfile(path) and not overwrite:
            with open(path, 'rb') as f:
                result_ds = np.load(f, allow_pickle=True).tolist()
            if 'time' in result_ds:
                result_ds[name + '_time'] = result_ds.pop('time')
            result.update(result_ds)
            continue
        rescale_features_factor = X.shape[1] / max_features if rescale_features and extend_features else 1.0
        extend_to = max(int(max_features), X.shape[1]) if extend_features else None
        start_time = time.time()
        ds_result = evaluate_dataset(X.to(device), y.to(device), categorical_feats, model, bptt, eval_position_range, rescale_features=rescale_features_factor,
                                     max_samples=max_samples, extend_to=extend_to)
        elapsed = time.time() - start_time
        for pos, (metric, outputs, ys) in zip(eval_position_range, ds_result):
            if save:
                result_ds[f'{name}_per_ds_metric_at_{pos}'] = metric
                result_ds[f'{name}_outputs_at_{pos}'] = outputs
                result_ds[f'{name}_ys_at_{pos}'] = ys.detach().cpu()
            flat = torch.as_tensor(outputs, dtype=torch.float32).reshape(-1, 1)
            if flat.shape[0] > hipops.AUC_MAX_ROWS:
                raise ValueError(f'{flat.shape[0]} pooled predictions at eval position {pos}: pfn_auc_counts takes up to {hipops.AUC_MAX_ROWS} rows per column; '
                                 f'lower max_samples')
            pooled, undefined = roc_auc_columns(flat.to(ys.device), ys.reshape(-1, 1))
            _report_undefined(undefined, f'pooled predictions of {name} at eval position {pos}')
            result_ds[f'{name}_mean_metric_at_{pos}'] = float(pooled[0])
            result_ds[name + '_time'] = elapsed
        if save and path is not None:
            os.makedirs(os.path.dirname(path), exist_ok=True)
            with open(path, 'wb') as f:
                np.save(f, result_ds)
        result.update(result_ds)
    for pos in eval_position_range:
        result[f'mean_metric_at_{pos}'] = np.array([result[f'{d[0]}_mean_metric_at_{pos}'] for d in datasets]).mean()
    result['mean_metric'] = np.array([result[f'mean_metric_at_{pos}'] for pos in eval_position_range]).mean()
    return result


def evaluate_dataset(X, y, categorical_feats, model, bptt, eval_position_range, plot=False, rescale_features=1.0, max_samples=40, extend_to=None):
    """Reference tabular.py:216-228: `evaluate_position` at every eval position; a list of its 3-tuples."""
    return [evaluate_position(X, y, categorical_feats, model, bptt, eval_position, rescale_features=rescale_features, max_samples=max_samples, extend_to=extend_to)
            for eval_position in eval_position_range]


def select_windows(num_rows, bptt, max_samples):
    """The reference's choice of windows (tabular.py:273-277): of the num_rows - bptt windows of bptt consecutive rows, the first `max_samples` of
    `torch.randperm` under seed 13, drawn on the CPU inside `fork_rng` so that the draw is the reference's and the caller's generator is left alone."""
    num_evals = num_rows - bptt
    if num_evals < 1:
        raise ValueError(f'a table of {num_rows} rows has no window of bptt = {bptt} rows (the reference takes len(X) - bptt windows)')
    with torch.random.fork_rng(devices=[]):
        torch.random.manual_seed(13)
        sel = torch.randperm(num_evals)
    return sel[:max_samples]


def pfn_window_logits(X, y, starts, model, bptt, eval_position, rescale_features=1.0, extend_to=None):
    """The PFN's logit for every test row of every window, [T, W] f32 on the GPU: window w is the table rows starts[w] .. starts[w] + bptt - 1, its first
    `eval_position` rows the training set.  One window launch and one forward in eval mode (`evaluate_position` says when it is more than one)."""
    sep = int(eval_position)
    T = int(bptt) - sep
    model.eval()
    F_out = X.shape[1] if extend_to is None else int(extend_to)
    per_call = max(1, MAX_TOKENS_PER_FORWARD // (T * (sep + 1)))
    logits = []
    with torch.no_grad():
        for w0 in range(0, len(starts), per_call):
            x_w, y_w = hipops.tabular_windows(X, y, starts[w0:w0 + per_call], bptt, sep, F_out=F_out, rescale=rescale_features, mode=hipops.TAB_NORM_WITH_TEST)
            logits.append(model((x_w, y_w), single_eval_pos=sep).reshape(-1, T))
    return torch.cat(logits, 0).t().contiguous()


def evaluate_position(X, y, categorical_feats, model, bptt, eval_position, rescale_features=1.0, max_samples=40, extend_to=None):
    """Reference tabular.py:231-306 for one eval position: returns (ROC-AUC per window [W] numpy, outputs [T, W] numpy f64, ys [T, W]) with T = bptt -
    eval_position test rows per window.  X [N, F], y [N] f32 on the GPU.
    PFN arm (`model` is an nn.Module): ONE pfn_tabular_windows launch builds all W T columns (train rows + one test row, normalised over those rows), ONE
    forward at batch W T in eval mode gives every logit, ONE pfn_auc_counts launch the metric.  The batch is split over several forwards only where it holds
    more than MAX_TOKENS_PER_FORWARD tokens, since the stack's workspace grows with the token count; the split is between windows and changes no number.
    Baseline arm (any other callable): `batch_pred`."""
    bptt, sep = int(bptt), int(eval_position)
    if not 1 <= sep < bptt:
        raise ValueError(f'eval position {sep} outside 1 .. bptt - 1 = {bptt - 1}')
    if X.dim() != 2 or y.shape != X.shape[:1]:
        raise ValueError('X [N, F], y [N]')
    starts = select_windows(X.shape[0], bptt, max_samples)
    W, T = len(starts), bptt - sep
    rows = (starts[:, None] + torch.arange(bptt)[None, :]).t().to(X.device)      # [bptt, W] table rows of every window
    X, y = X.float().contiguous(), y.float().contiguous()
    ys = y[rows[sep:]]
    if isinstance(model, nn.Module):
        scores = torch.sigmoid(pfn_window_logits(X, y, starts, model, bptt, sep, rescale_features=rescale_features, extend_to=extend_to))      # [T, W]
        metric, undefined = roc_auc_columns(scores, ys)
        _report_undefined(undefined, f'of {W} windows at eval position {sep}')
        return metric, scores.double().cpu().numpy(), ys
    eval_xs = X[rows]
    if extend_to is not None and extend_to > X.shape[1]:
        eval_xs = torch.cat([eval_xs, eval_xs.new_zeros(bptt, W, int(extend_to) - X.shape[1])], -1)
    metric, outputs = batch_pred(model, eval_xs, y[rows], categorical_feats, start=sep, table=(X, y, starts, extend_to))
    return metric, outputs, ys


def batch_pred(metric_function, eval_xs, eval_ys, categorical_feats, start=2, table=None):
    """Reference tabular.py:309-323: normalise every window eval_xs[:, w] [bptt, F] by the mean and std of its first `start` rows and hand
    (train x, train y, test x, test y, categorical_feats) to the metric function; returns (metrics [W], outputs [T, W]).  A metric function with a `batched`
    form (`knn_metric`) gets all windows at once; any other callable is looped window by window as the reference loops, on torch's normalisation.  `table` =
    (X, y, starts, extend_to), when the windows are slices of one table, lets the batched form gather and normalise them in one pfn_tabular_windows launch."""
    batched = getattr(metric_function, 'batched', None)
    if batched is not None and eval_xs.is_cuda:
        if table is not None:
            X, y, starts, extend_to = table
            x, _ = hipops.tabular_windows(X, y, starts, eval_xs.shape[0], start, F_out=X.shape[1] if extend_to is None else int(extend_to),
                                          mode=hipops.TAB_NORM_TRAIN_ONLY)
        else:      # windows that are no slices of a table: window w is the table's rows w bptt .. (w + 1) bptt - 1
            bptt, W, F = eval_xs.shape
            flat = eval_xs.float().transpose(0, 1).reshape(W * bptt, F).contiguous()
            x, _ = hipops.tabular_windows(flat, eval_ys.float().t().reshape(-1).contiguous(), [w * bptt for w in range(W)], bptt, start, mode=hipops.TAB_NORM_TRAIN_ONLY)
        return batched(x[:start], eval_ys[:start], x[start:], eval_ys[start:])
    metrics, outputs = [], []
    for eval_x, eval_y in zip(eval_xs.transpose(0, 1), eval_ys.transpose(0, 1)):
        mean = eval_x[:start].mean(0)
        std = eval_x[:start].std(0) + .000001
        eval_x = (eval_x - mean) / std
        metric, output = metric_function(eval_x[:start], eval_y[:start], eval_x[start:], eval_y[start:], categorical_feats)
        metrics += [metric]
        outputs += [output]
    return np.array(metrics), np.array(outputs).T


## What the baseline arms share (kNN, logistic regression, GP classifier), each arm handing in what is its own: the problems before the launch, GridSearchCV's
## ranking, the tail after the selection, the single-problem form

def _fold_problems(x, y, test_x, one_class_error=None, n_splits=None):
    """Before the launch, for W problems: x [n, W, F] normalised train rows, y [n, W], test_x [T, W, F] -> (n_splits = min(CV, n // 2), folds [W, n] int32: every
    row's test fold, cls [n, W] bool: label > 0.5, both on the host, and the kernels' operands on x's device: (train [W, n, F], labels [W, n], test [W, T, F] f32,
    fold [W, n] int32)).  one_class_error: the arm's name where a window whose train rows hold one class raises ValueError, as scikit-learn's fit does.
    n_splits: the number of folds where the arm does not take min(CV, n // 2) (xgb_metric passes cv=5 whatever n is)."""
    n, W, _ = x.shape
    n_splits = min(CV, n // 2) if n_splits is None else int(n_splits)
    cls = y.detach().cpu().numpy() > 0.5
    if one_class_error is not None:
        for w in range(W):
            if cls[:, w].all() or not cls[:, w].any():
                raise ValueError(f'{one_class_error}_metric: the train rows of window {w} hold one class only')
    folds = np.stack([_stratified_folds(cls[:, w], n_splits) for w in range(W)])
    return n_splits, folds, cls, (x.float().transpose(0, 1).contiguous(), y.float().t().contiguous(), test_x.float().transpose(0, 1).contiguous(),
                                  torch.from_numpy(folds).to(x.device))


def _fold_sizes(folds, n_splits):
    """The rows in every test fold of one problem, f64 [n_splits]: what a fold's count of correct rows is divided by."""
    return np.bincount(np.asarray(folds), minlength=n_splits)[:n_splits].astype(np.float64)


def _first_maximum(scores, all_failed_error=None):
    """GridSearchCV's ranking of one problem: scores [candidates, n_splits] f64, NaN where a fit did not run -> (mean_test_score [candidates], index of the best:
    the FIRST maximum, NaN ranks last).  all_failed_error: the arm's name where scores that are all NaN raise ValueError; without it candidate 0 wins then."""
    if all_failed_error is not None and np.isnan(scores).all():
        raise ValueError(f'{all_failed_error}_metric: every fit of every candidate failed (each fold\'s training part holds one class)')
    mean = scores.mean(axis=1)
    return mean, int(np.argmax(np.where(np.isnan(mean), -np.inf, mean)))


def _fold_metric(chosen, test_y):
    """After the selection: chosen = per problem (mean_test_score, best, proba [T] f64), test_y [T, W] on the GPU -> (ROC-AUC [W], proba [T, W]) numpy."""
    proba = np.stack([c[2] for c in chosen], 1)
    metric, undefined = roc_auc_columns(torch.from_numpy(proba).float().to(test_y.device), test_y)
    _report_undefined(undefined, f'of {len(chosen)} windows')
    return metric, proba


def _single_problem(batched):
    """Decorator that gives a documented metric function (x [n, F], y [n], test_x [T, F], test_y [T], cat_features) -> (metric, proba [T]) its body: the batched
    form on one problem.  The batched form itself is attached as `.batched`; `batch_pred` uses it."""
    def build(documented):
        @functools.wraps(documented)
        def metric_function(x, y, test_x, test_y, cat_features):
            metric, proba = batched(x[:, None], y[:, None], test_x[:, None], test_y[:, None])
            return metric[0], proba[:, 0]
        metric_function.batched = batched
        return metric_function
    return build


## KNN (reference tabular.py:349-369)

def _stratified_folds(y, n_splits):
    """The test fold of every sample under sklearn's `StratifiedKFold(n_splits, shuffle=False)` (its `_make_test_folds`): classes numbered by first
    appearance, the sorted labels dealt round-robin over the folds to fix how many samples of each class a fold gets, then each class's samples assigned to
    the folds in blocks, in data order.  Raises ValueError where sklearn does (fewer than 2 splits, more splits than samples, more splits than members in
    EVERY class); where sklearn only warns (more splits than members in SOME class) it goes on, silently.  Returns int32 [n]."""
    y = np.asarray(y).reshape(-1)
    n_splits = int(n_splits)
    if n_splits < 2:
        raise ValueError(f'k-fold cross-validation requires at least one train/test split: n_splits={n_splits}')
    if n_splits > len(y):
        raise ValueError(f'Cannot have number of splits n_splits={n_splits} greater than the number of samples: n_samples={len(y)}.')
    _, first, inverse = np.unique(y, return_index=True, return_inverse=True)
    _, by_appearance = np.unique(first, return_inverse=True)
    encoded = by_appearance[inverse.reshape(-1)]
    n_classes = len(first)
    counts = np.bincount(encoded)
    if np.all(n_splits > counts):
        raise ValueError(f'n_splits={n_splits} cannot be greater than the number of members in each class.')
    ordered = np.sort(encoded)
    allocation = np.asarray([np.bincount(ordered[i::n_splits], minlength=n_classes) for i in range(n_splits)])
    folds = np.empty(len(y), dtype=np.int32)
    for k in range(n_classes):
        folds[encoded == k] = np.arange(n_splits).repeat(allocation[:, k])
    return folds


def _knn_grid(n):
    """(candidate k values, number of folds) of the reference's grid search on n train rows: k = 1 .. min(5, n - 2), cv = min(CV, n // 2)."""
    return np.arange(1, min(6, n - 1)), min(CV, n // 2)


def _knn_select(cv_correct, folds, n_splits, ks, test_pos):
    """The host half of one problem's grid search, from the kernel's integer counts: cv_correct [5, 5] (k - 1, fold), folds [n] the rows' test folds,
    test_pos [T, 5].  As GridSearchCV(KNeighborsClassifier(), {'n_neighbors': ks}, cv=n_splits) scores it: a fold's score is its accuracy correct / size in
    f64 -- NaN where k exceeds the fold's training rows (the fit fails, error_score = nan) --, a candidate's score the mean over folds, the best candidate the
    FIRST maximum (NaN ranks last), the refit on all rows gives predict_proba[:, 1] = positives among the k* nearest / k*.
    Returns (mean_test_score [len(ks)] f64, best k, proba [T] f64)."""
    sizes = _fold_sizes(folds, n_splits)
    correct = np.asarray(cv_correct, dtype=np.float64)
    scores = np.empty((len(ks), n_splits), dtype=np.float64)
    for i, k in enumerate(ks):
        scores[i] = correct[k - 1, :n_splits] / sizes
        scores[i, sizes.sum() - sizes < k] = np.nan
    mean, first = _first_maximum(scores)
    best = int(ks[first])
    proba = np.asarray(test_pos, dtype=np.float64)[:, best - 1] / float(best)
    return mean, best, proba


def _knn_batched(x, y, test_x, test_y, return_k=False):
    """kNN with its grid search for W problems at once: x [n, W, F] normalised train rows, y [n, W], test_x [T, W, F], test_y [T, W] on the GPU.  One
    pfn_knn_cv launch finds every neighbour list; the folds (before) and the scores (after) are host arithmetic.  Returns (ROC-AUC [W], proba [T, W]) numpy,
    and with return_k the chosen k of every problem as a third entry."""
    n, W, F = x.shape
    hipops.knn_cv_check(n, test_x.shape[0], F)
    ks, _ = _knn_grid(n)
    n_splits, folds, _, operands = _fold_problems(x, y, test_x)
    cv_correct, test_pos, _ = hipops.knn_cv(*operands)
    cv_correct, test_pos = cv_correct.cpu().numpy(), test_pos.cpu().numpy()
    chosen = [_knn_select(cv_correct[w], folds[w], n_splits, ks, test_pos[w]) for w in range(W)]
    metric, proba = _fold_metric(chosen, test_y)
    return (metric, proba, [c[1] for c in chosen]) if return_k else (metric, proba)


@_single_problem(_knn_batched)
def knn_metric(x, y, test_x, test_y, cat_features):
    """Reference tabular.py:351-369 for one problem: x [n, F] (normalised) train rows, y [n], test_x [T, F], test_y [T] on the GPU -> (ROC-AUC, proba [T]) of
    a KNeighborsClassifier whose k is grid-searched over 1 .. min(5, n - 2) by min(5, n // 2)-fold stratified cross-validation.  `knn_metric.batched` is the
    same for many problems in one launch; `batch_pred` uses it."""


## Logistic regression (reference tabular.py:325-346)

param_grid = {}
param_grid['logistic'] = {'solver': ['saga'], 'penalty': ['l1', 'l2', 'none'], 'tol': [1e-2, 1e-4, 1e-10], 'max_iter': [500], 'fit_intercept': [True, False],
                          'C': [1e-5, 0.001, 0.01, 0.1, 1.0, 2.0]}


def _logistic_grid(grid=None):
    """The reference's grid as the device solves it: (entries, cands, entry_fit).  `entries` are the parameter dicts in sklearn's ParameterGrid order (keys
    sorted, the last key varying fastest: 108 of them); `cands` the distinct fits [(C, penalty code | fit-intercept bit)] in order of first appearance -- tol,
    max_iter and solver do not change a fit that is solved to its optimum, and 'none' ignores C (1 stands in): 26 --; entry_fit [entries] indexes `cands`."""
    import itertools
    grid = param_grid['logistic'] if grid is None else grid
    keys = sorted(grid)
    entries = [dict(zip(keys, values)) for values in itertools.product(*(grid[k] for k in keys))]
    cands, entry_fit, where = [], [], {}
    for e in entries:
        penalty = hipops.LOGIT_PENALTIES[e['penalty']]
        key = (1.0 if penalty == hipops.LOGIT_NONE else float(e['C']), penalty | (hipops.LOGIT_FIT_INTERCEPT if e['fit_intercept'] else 0))
        if key not in where:
            where[key] = len(cands)
            cands.append(key)
        entry_fit.append(where[key])
    return entries, cands, np.asarray(entry_fit)


def _logistic_select(cv_correct, status, folds, n_splits, entry_fit, test_z):
    """The host half of one problem's grid search, from the kernel's results: cv_correct [NC, 5] counts, status [NC, 6, 2], folds [n] the rows' test folds,
    entry_fit [entries] the fit of every grid entry, test_z [NC, T] the refits' decision values.  As GridSearchCV scores it: a fold's score is its accuracy
    correct / size in f64 -- NaN where the fold's training part holds one class (the fit fails, error_score = nan) --, a candidate's score the mean over folds,
    the best entry the FIRST maximum over the full entry order (NaN ranks last; where a failed fold leaves every mean NaN that is entry 0, as in sklearn),
    predict_proba[:, 1] = sigmoid(decision value of its refit) in f64.
    Returns (mean_test_score [entries] f64, best entry index, proba [T] f64); raises ValueError when every fit of every candidate failed."""
    scores = np.asarray(cv_correct, dtype=np.float64)[:, :n_splits] / _fold_sizes(folds, n_splits)
    scores[np.asarray(status)[:, :n_splits, 0] == hipops.LOGIT_ONE_CLASS] = np.nan
    mean, best = _first_maximum(scores[np.asarray(entry_fit)], all_failed_error='logistic')      # every entry has the scores of its fit
    z = np.asarray(test_z, dtype=np.float64)[entry_fit[best]]
    e = np.exp(-np.abs(z))
    proba = np.where(z >= 0, 1 / (1 + e), e / (1 + e))
    return mean, best, proba


def _logistic_batched(x, y, test_x, test_y, return_params=False):
    """Logistic regression with the reference's grid search for W problems at once: x [n, W, F] normalised train rows, y [n, W], test_x [T, W, F], test_y [T, W]
    on the GPU.  One pfn_logistic_cv launch solves all W x 26 x (folds + 1) fits; the folds (before) and the scores (after) are host arithmetic.  Returns
    (ROC-AUC [W], proba [T, W]) numpy, and with return_params the chosen parameter dict of every problem as a third entry.  Raises ValueError, as sklearn's fit
    does, for a window whose train rows hold one class."""
    n, W, F = x.shape
    entries, cands, entry_fit = _logistic_grid()
    hipops.logistic_cv_check(n, test_x.shape[0], F, len(cands))
    n_splits, folds, _, operands = _fold_problems(x, y, test_x, one_class_error='logistic')
    cv_correct, test_z, status, _ = hipops.logistic_cv(*operands, n_splits, [c for c, _ in cands], [k for _, k in cands])
    cv_correct, test_z, status = cv_correct.cpu().numpy(), test_z.cpu().numpy(), status.cpu().numpy()
    chosen = [_logistic_select(cv_correct[w], status[w], folds[w], n_splits, entry_fit, test_z[w]) for w in range(W)]
    metric, proba = _fold_metric(chosen, test_y)
    return (metric, proba, [entries[c[1]] for c in chosen]) if return_params else (metric, proba)


@_single_problem(_logistic_batched)
def logistic_metric(x, y, test_x, test_y, cat_features):
    """Reference tabular.py:326-346 for one problem: x [n, F] (normalised) train rows, y [n], test_x [T, F], test_y [T] on the GPU -> (ROC-AUC, proba [T]) of
    the LogisticRegression that GridSearchCV picks from param_grid['logistic'] by min(5, n // 2)-fold stratified cross-validation, every candidate solved to its
    optimum.  `logistic_metric.batched` is the same for many problems in one launch; `batch_pred` uses it."""


## GP classifier (reference tabular.py:480-503)

param_grid['gp'] = {'params_y_scale': [0.05, 0.1, 0.5, 1.0, 5.0, 10.0], 'params_length_scale': [0.1, 0.5, 1.0, 2.0]}      # the kernels are c * RBF(l) over their product
GP_BOX = (float(np.log(1e-5)), float(np.log(1e5)))      # scikit-learn's default bounds of both hyper-parameters, in theta = log
GP_LBFGS = dict(gtol=1e-3, ftol=1e-6, max_iter=100)     # sized to the f32 objective (INTEGRATION.md has scikit-learn's beside them)
# Williams & Barber's five-term erf approximation of the logistic sigmoid, as scikit-learn's predict_proba uses it
_GP_LAMBDAS = (0.41, 0.4, 0.37, 0.44, 0.39)
_GP_COEFS = (-1854.8214151, 3516.89893646, 221.29346712, 128.12323805, -2010.49422654)


def _gp_grid(grid=None):
    """The reference's 24 candidate kernels c * RBF(l) as (c, l) pairs in its order, `itertools.product` over (c values, l values)."""
    import itertools
    grid = param_grid['gp'] if grid is None else grid
    return [(float(c), float(l)) for c, l in itertools.product(grid['params_y_scale'], grid['params_length_scale'])]


def _gp_proba(f_star, var):
    """scikit-learn's predict_proba[:, 1] from the latent mean and variance, in f64: sum_k coef_k 1/2 erf(lambda_k f* / sqrt(1 + 2 var lambda_k^2)) + 1/2 sum_k
    coef_k -- its expression with alpha = 1 / (2 var) multiplied out, so that the var = 0 the kernel clamps to is an ordinary argument."""
    f_star, var = torch.as_tensor(f_star, dtype=torch.float64), torch.as_tensor(var, dtype=torch.float64).clamp_min(0)
    lam, coef = torch.tensor(_GP_LAMBDAS, dtype=torch.float64)[:, None], torch.tensor(_GP_COEFS, dtype=torch.float64)[:, None]
    integrals = 0.5 * torch.erf(lam * f_star / torch.sqrt(1 + 2 * var * lam ** 2))
    return ((coef * integrals).sum(0) + 0.5 * coef.sum()).numpy()


def _gp_f_star(pairs):
    """The decision values of the kernel's (m, e) pairs [..., 2], formed in f64: f* = m exp(-e)."""
    pairs = np.asarray(pairs, dtype=np.float64)
    return pairs[..., 0] * np.exp(-pairs[..., 1])


def _gp_select(cv_f, status, folds, y, n_splits, test_f, test_var):
    """The host half of one problem's grid search, in f64, from the kernel's results: cv_f [NC, n, 2] the (m, e) pair of every row from the fit that held it
    out, status [NC, 6, 2], folds [n] the rows' test folds, y [n] the labels, test_f [NC, T, 2] and test_var [NC, T] of the refits.  As GridSearchCV scores it:
    a fold's score is the accuracy of (f* > 0) on its rows -- NaN where the fit did not run or failed (a one-class training part: the fit raises, error_score =
    nan) --, a candidate's score the mean over folds, the best candidate the FIRST maximum (NaN ranks last), predict_proba[:, 1] the erf mixture of its refit.
    Returns (mean_test_score [NC] f64, best index, proba [T] f64); raises ValueError when every fit of every candidate failed."""
    folds, cls = np.asarray(folds), np.asarray(y) > 0.5
    reasons = np.asarray(status)[:, :n_splits, 0]
    ran = (reasons == hipops.GPC_CONVERGED) | (reasons == hipops.GPC_CAPPED)
    right = (_gp_f_star(cv_f) > 0) == cls[None, :]      # [NC, n]
    sizes = _fold_sizes(folds, n_splits)
    scores = np.full(ran.shape, np.nan)
    for s in range(n_splits):
        scores[:, s] = np.where(ran[:, s], right[:, folds == s].sum(1) / sizes[s], np.nan)
    mean, best = _first_maximum(scores, all_failed_error='gp')
    return mean, best, _gp_proba(_gp_f_star(np.asarray(test_f)[best]), np.asarray(test_var)[best])


def _gp_objective(x, y, folds, n_splits, shape, counters=None):
    """-Z and its gradient for batched_lbfgs, all fits of the call in one pfn_gpc_lml_grad launch.  The box is applied here: the kernel sees the clipped theta,
    and a gradient component that points out of the box at a bound is zero."""
    lo, hi = GP_BOX

    def fun(theta):
        inside = theta.clamp(lo, hi)
        value, grad, _ = hipops.gpc_lml_grad(inside.reshape(shape).contiguous(), x, y, folds, n_splits)
        grad = grad.reshape(-1, 2)
        out = ((theta <= lo) & (grad > 0)) | ((theta >= hi) & (grad < 0))
        if counters is not None:
            counters['passes'] = counters.get('passes', 0) + 1
        return value.reshape(-1), torch.where(out, torch.zeros_like(grad), grad)
    return fun


def _gp_batched(x, y, test_x, test_y, optimize=True, return_params=False, counters=None):
    """The GP classifier with the reference's grid search for W problems at once: x [n, W, F] normalised train rows, y [n, W], test_x [T, W, F], test_y [T, W] on
    the GPU.  Every one of the W x 24 x (folds + 1) fits starts at its candidate's theta = (log c, log l) and maximises its own Laplace log marginal likelihood
    by `batched_lbfgs` inside the box GP_BOX, every pass ONE pfn_gpc_lml_grad launch; one pfn_gpc_predict launch at the final thetas gives the decision values;
    the folds (before) and the scores, the selection and the probabilities (after) are host arithmetic in f64.  `optimize=False` skips the optimiser: every
    candidate is fitted at its own theta (scikit-learn's optimizer=None).  Returns (ROC-AUC [W], proba [T, W]) numpy, and with return_params a third entry: per
    problem dict(kernel=(c, l) of the chosen refit after optimisation, start=(c, l) of its candidate, index).  `counters`, a dict, receives the L-BFGS pass
    count and the fits' exit reasons.  Raises ValueError, as scikit-learn's fit does, for a window whose train rows hold one class."""
    n, W, F = x.shape
    cands = _gp_grid()
    NC = len(cands)
    hipops.gpc_check(n, test_x.shape[0], F, NC)
    n_splits, folds, cls, (xs, ys, ts, folds_dev) = _fold_problems(x, y, test_x, one_class_error='gp')
    shape = (W, NC, hipops.GPC_SLOTS, 2)
    theta = torch.tensor(cands, dtype=torch.float64).log().float().to(x.device)[None, :, None, :].expand(shape).contiguous()
    if optimize:
        res = priors.fast_gp_mix.batched_lbfgs(_gp_objective(xs, ys, folds_dev, n_splits, shape, counters), theta.reshape(-1, 2), **GP_LBFGS)
        theta = res['theta'].clamp(*GP_BOX).reshape(shape).contiguous()
        if counters is not None:
            counters['converged'] = res['converged'].reshape(shape[:3])[:, :, :n_splits + 1].cpu().numpy()
            counters['objective'] = res['objective'].reshape(shape[:3])[:, :, :n_splits + 1].double().cpu().numpy()
            counters['evaluations'] = res['evaluations']
    cv_f, test_f, test_var, status = hipops.gpc_predict(theta, xs, ys, ts, folds_dev, n_splits)
    cv_f, test_f, test_var, status, theta_host = cv_f.cpu().numpy(), test_f.cpu().numpy(), test_var.cpu().numpy(), status.cpu().numpy(), theta.double().cpu().numpy()
    if counters is not None:
        counters['status'] = status
        counters['theta'] = theta_host
    y01 = cls.astype(np.float64)
    chosen = [_gp_select(cv_f[w], status[w], folds[w], y01[:, w], n_splits, test_f[w], test_var[w]) for w in range(W)]
    metric, proba = _fold_metric(chosen, test_y)
    if not return_params:
        return metric, proba
    params = [dict(kernel=tuple(float(v) for v in np.exp(theta_host[w, c[1], n_splits])), start=cands[c[1]], index=c[1]) for w, c in enumerate(chosen)]
    return metric, proba, params


@_single_problem(_gp_batched)
def gp_metric(x, y, test_x, test_y, cat_features):
    """Reference tabular.py:480-503 for one problem: x [n, F] (normalised) train rows, y [n], test_x [T, F], test_y [T] on the GPU -> (ROC-AUC, proba [T]) of
    the GaussianProcessClassifier that GridSearchCV picks from the 24 kernels c * RBF(l) of param_grid['gp'] by min(5, n // 2)-fold stratified cross-validation
    (INTEGRATION.md).  `gp_metric.batched` is the same for many problems at once; `batch_pred` uses it."""


## BNN classifier (reference tabular.py:372-478)

param_grid['bayes'] = {'embed': [5, 10, 30, 64], 'lr': [1e-3, 1e-4], 'num_training_steps': [400], 'num_samples_for_prediction': [400]}
BAYES_INIT_DRAWS = 15       # pyro's init_to_median: the start is the median of 15 prior draws per coordinate
BAYES_INIT_SCALE = 0.1      # AutoDiagonalNormal's init_scale


def _bayes_grid(grid=None):
    """The reference's grid as the device runs it: (entries, cands, num_steps, num_draws).  `entries` are the parameter dicts in sklearn's ParameterGrid order
    (keys sorted, the last key varying fastest: (5, 1e-3), (5, 1e-4), (10, 1e-3), ..., (64, 1e-4)), `cands` their (embed, lr).  'num_training_steps' and
    'num_samples_for_prediction' are no constructor arguments of the reference's estimator -- its GridSearchCV raises on them --; each holds one
    value, which is read here and applied as the step count and the draw count of every candidate."""
    import itertools
    grid = param_grid['bayes'] if grid is None else grid
    if len(grid['num_training_steps']) != 1 or len(grid['num_samples_for_prediction']) != 1:
        raise ValueError("param_grid['bayes']: 'num_training_steps' and 'num_samples_for_prediction' hold one value each")
    keys = sorted(grid)
    entries = [dict(zip(keys, values)) for values in itertools.product(*(grid[k] for k in keys))]
    return entries, [(int(e['embed']), float(e['lr'])) for e in entries], int(grid['num_training_steps'][0]), int(grid['num_samples_for_prediction'][0])


def _bayes_select(cv_prob, folds, cls, n_splits, test_prob):
    """The host half of one problem's grid search, in f64: cv_prob [NC, n] every train row's class-1 probability from the fit that held it out, folds [n] the rows'
    test folds, cls [n] bool, test_prob [NC, T] of the refits.  As GridSearchCV scores it: a fold's score is the share of its rows with (prob > 0.5) == class
    (prob exactly 0.5 predicts class 0), a candidate's score the mean over folds, the best candidate the FIRST maximum (NaN ranks last).
    Returns (mean_test_score [NC] f64, best index, proba [T] f64)."""
    cv_prob, folds, cls = np.asarray(cv_prob, dtype=np.float64), np.asarray(folds), np.asarray(cls, dtype=bool)
    right = (cv_prob > 0.5) == cls[None, :]
    sizes = _fold_sizes(folds, n_splits)
    scores = np.stack([right[:, folds == s].sum(1) / sizes[s] for s in range(n_splits)], 1)
    scores[np.stack([np.isnan(cv_prob[:, folds == s]).any(1) for s in range(n_splits)], 1)] = np.nan      # a fit that left the finite numbers
    mean, best = _first_maximum(scores)
    return mean, best, np.asarray(test_prob, dtype=np.float64)[best]


def _bayes_loc0(seed, problem, cand, D):
    """The initial loc of the six slots of one (problem, candidate), [6, D] f32 on the host: the median of 15 N(0, 1) draws per coordinate (pyro's init_to_median
    under this prior, as `fit_bnn_svi`), from a generator of its own, so that a fit's start depends on (seed, problem index, candidate index) alone."""
    g = torch.Generator().manual_seed((int(seed) * 1000003 + int(problem)) * hipops.BNN_CV_MAX_CANDIDATES + int(cand))
    return torch.randn(BAYES_INIT_DRAWS, hipops.BNN_CV_SLOTS, int(D), generator=g).median(0).values


def _bayes_batched(x, y, test_x, test_y, return_params=False, sample_obs=False, seed=0, details=None):
    """The BNN classifier with the reference's grid search for W problems at once: x [n, W, F] normalised train rows, y [n, W], test_x [T, W, F], test_y [T, W] on
    the GPU.  One pfn_bnn_cv launch runs the 400 SVI steps and the 400 predictive draws of all W x 8 x (folds + 1) fits; the folds and the starts (before) and the
    scores and the selection (after) are host arithmetic.  The returned probability is the mean over the draws of the class-1 probability; sample_obs=True gives
    the reference's estimator instead, the mean of one sampled observation per draw (the convention of `eval_mcmc` / `eval_svi`); the selection always uses the
    former.  Returns (ROC-AUC [W], proba [T, W]) numpy, and with return_params the chosen parameter dict of every problem as a third entry.  `details`, a dict,
    receives the launch's cv_prob, test_prob, status and per-step loss, the folds and every problem's (mean_test_score, best)."""
    n, W, F = x.shape
    entries, cands, num_steps, num_draws = _bayes_grid()
    cand_H, cand_lr = [h for h, _ in cands], [lr for _, lr in cands]
    hipops.bnn_cv_check(n, test_x.shape[0], F, cand_H)
    if not x.is_cuda:
        raise NotImplementedError('bayes_net_metric runs on the GPU only (pfn_bnn_cv); there is no CPU path')
    n_splits, folds, cls, operands = _fold_problems(x, y, test_x)
    state = hipops.bnn_cv_state(W, cand_H, F, x.device, init_scale=BAYES_INIT_SCALE)
    for c, H in enumerate(cand_H):      # candidate by candidate: the host transient is one candidate's draws
        D = hipops.bnn_num_params(F, H)
        state[:, c, :, 0, :D] = torch.stack([_bayes_loc0(seed, w, c, D) for w in range(W)]).to(x.device)
    out = hipops.bnn_cv(*operands, n_splits, cand_H, cand_lr, state, num_steps, num_pred_samples=num_draws, seed=seed, sample_obs=sample_obs,
                        want_loss=details is not None)
    cv_prob, test_prob = out.cv_prob.double().cpu().numpy(), out.test_prob.double().cpu().numpy()
    reported = out.test_draw.double().cpu().numpy() if sample_obs else test_prob
    chosen = [_bayes_select(cv_prob[w], folds[w], cls[:, w], n_splits, reported[w]) for w in range(W)]
    if details is not None:
        details.update(cv_prob=cv_prob, test_prob=test_prob, status=out.status.cpu().numpy(), loss=out.loss.cpu().numpy(), folds=folds, n_splits=n_splits,
                       scores=[(c[0], c[1]) for c in chosen])
    metric, proba = _fold_metric(chosen, test_y)
    return (metric, proba, [entries[c[1]] for c in chosen]) if return_params else (metric, proba)


@_single_problem(_bayes_batched)
def bayes_net_metric(x, y, test_x, test_y, cat_features):
    """Reference tabular.py:465-478 for one problem: x [n, F] (normalised) train rows, y [n], test_x [T, F], test_y [T] on the GPU -> (ROC-AUC, proba [T]) of the
    two-layer Bayesian neural network (fc1 -> fc2, N(0, 1) priors, mean-field Gaussian guide, 400 Adam steps on the ELBO, 400 predictive draws) that a grid search
    over param_grid['bayes'] picks by min(5, n // 2)-fold stratified cross-validation.  `bayes_net_metric.batched` is the same for
    many problems in one launch; `batch_pred` uses it."""


## Gradient-boosted trees (reference tabular.py:599-626)

param_grid['xgb'] = {'min_child_weight': [0.5, 1.0], 'learning_rate': [0.02, 0.2], 'subsample': [0.5, 0.8], 'max_depth': [1, 2], 'colsample_bytree': [0.8],
                     'eval_metric': ['logloss'], 'n_estimators': [100]}
XGB_FOLDS = 5      # the reference passes cv=5, not min(CV, n // 2)


def _xgb_grid(grid=None):
    """The reference's grid as the device runs it: (entries, num_rounds).  `entries` are the parameter dicts in sklearn's ParameterGrid order (keys sorted, the
    last key varying fastest: subsample, then min_child_weight, max_depth, learning_rate).  'n_estimators' and 'colsample_bytree' are read from the entry --
    'n_estimators' holds one value, a launch has one round count --, 'eval_metric' is accepted and ignored: it scores nothing here."""
    import itertools
    grid = param_grid['xgb'] if grid is None else grid
    if len(grid['n_estimators']) != 1:
        raise ValueError("param_grid['xgb']: 'n_estimators' holds one value")
    keys = sorted(grid)
    entries = [dict(zip(keys, values)) for values in itertools.product(*(grid[k] for k in keys))]
    return entries, int(grid['n_estimators'][0])


def _xgb_select(cv_margin, folds, cls, n_splits, test_margin):
    """The host half of one problem's grid search, in f64: cv_margin [NC, n] every train row's final margin from the fit that held it out, folds [n] the rows'
    test folds, cls [n] bool, test_margin [NC, T] of the refits.  As GridSearchCV scores an XGBClassifier: a fold's score is the share of its rows with
    (margin > 0) == class (proba exactly 0.5 predicts class 0), a candidate's score the mean over folds, the best candidate the FIRST maximum (NaN ranks last).
    Returns (mean_test_score [NC] f64, best index, proba [T] f64 = sigmoid(margin) of the best candidate's refit)."""
    cv_margin, folds, cls = np.asarray(cv_margin, dtype=np.float64), np.asarray(folds), np.asarray(cls, dtype=bool)
    right = (cv_margin > 0) == cls[None, :]
    sizes = _fold_sizes(folds, n_splits)
    scores = np.stack([right[:, folds == s].sum(1) / sizes[s] for s in range(n_splits)], 1)
    scores[np.stack([np.isnan(cv_margin[:, folds == s]).any(1) for s in range(n_splits)], 1)] = np.nan      # a fit that left the finite numbers
    mean, best = _first_maximum(scores)
    return mean, best, 1. / (1. + np.exp(-np.asarray(test_margin, dtype=np.float64)[best]))


def _xgb_batched(x, y, test_x, test_y, return_params=False, seed=0, details=None):
    """Gradient-boosted trees with the reference's grid search for W problems at once: x [n, W, F] normalised train rows, y [n, W], test_x [T, W, F], test_y [T, W]
    on the GPU.  One pfn_xgb_cv launch runs the 100 rounds of all W x 16 x 6 fits; the 5 stratified folds (before) and the scores and the selection (after) are
    host arithmetic.  Returns (accuracy [W] -- ((proba > 0.5) == test_y).mean() as the reference's xgb_metric computes it, not ROC-AUC --, proba [T, W]) numpy, and
    with return_params the chosen parameter dict of every problem as a third entry.  `details`, a dict, receives the launch's margins, status and trees, the folds
    and every problem's (mean_test_score, best)."""
    n, W, F = x.shape
    entries, num_rounds = _xgb_grid()
    depth = [int(e['max_depth']) for e in entries]
    hipops.xgb_cv_check(n, test_x.shape[0], F, depth, num_rounds)
    if not x.is_cuda:
        raise NotImplementedError('xgb_metric runs on the GPU only (pfn_xgb_cv); there is no CPU path')
    n_splits, folds, cls, operands = _fold_problems(x, y, test_x, n_splits=XGB_FOLDS)
    out = hipops.xgb_cv(*operands, n_splits, depth, [e['learning_rate'] for e in entries], [e['min_child_weight'] for e in entries],
                        [e['subsample'] for e in entries], [e['colsample_bytree'] for e in entries], num_rounds, seed=seed, want_trees=details is not None)
    cv_margin, test_margin = out.cv_margin.double().cpu().numpy(), out.test_margin.double().cpu().numpy()
    chosen = [_xgb_select(cv_margin[w], folds[w], cls[:, w], n_splits, test_margin[w]) for w in range(W)]
    if details is not None:
        details.update(cv_margin=cv_margin, test_margin=test_margin, status=out.status.cpu().numpy(), folds=folds, n_splits=n_splits,
                       trees=tuple(t.cpu().numpy() for t in out[3:]), scores=[(c[0], c[1]) for c in chosen])
    proba = np.stack([c[2] for c in chosen], 1)
    metric = ((proba > 0.5) == (test_y.detach().cpu().numpy() > 0.5)).astype(np.float64).mean(0)
    return (metric, proba, [entries[c[1]] for c in chosen]) if return_params else (metric, proba)


@_single_problem(_xgb_batched)
def xgb_metric(x, y, test_x, test_y, cat_features):
    """Reference tabular.py:610-626 for one problem: x [n, F] (normalised) train rows, y [n], test_x [T, F], test_y [T] on the GPU -> (accuracy, proba [T]) of the
    gradient-boosted trees (exact greedy splits, logistic loss, 100 rounds) that a grid search over param_grid['xgb'] picks by 5-fold stratified cross-validation
    (INTEGRATION.md).  cat_features is accepted and ignored, as in the reference's call.  `xgb_metric.batched` is the same for many problems in one
    launch; `batch_pred` uses it."""


## CatBoost (reference tabular.py:556-596)

param_grid['catboost'] = {'learning_rate': [0.1, 0.5, 1.0], 'depth': [2, 4, 7], 'l2_leaf_reg': [0.0, 0.5, 1], 'iterations': [10, 40, 70]}
CATBOOST_HOLDOUT = 0.2      # grid_search's train_size = 0.8


def _catboost_grid(grid=None):
    """The reference's grid as the device runs it: (entries, fits, where, checkpoints).  `entries` are the 81 parameter dicts in the order CatBoost's grid_search
    walks them: the dict's key order, the last key ('iterations') varying fastest.  Nothing in a fit depends on 'iterations' -- tree t is grown from the margins
    after tree t - 1 and from draws addressed by t --, so a fit of 70 trees contains those of 10 and 40 as prefixes: `fits` are the 27 distinct (learning_rate,
    depth, l2_leaf_reg) in order of first appearance, `where[e]` = (fit, checkpoint) of entry e, `checkpoints` the ascending tree counts (10, 40, 70)."""
    import itertools
    grid = param_grid['catboost'] if grid is None else grid
    keys = list(grid)
    entries = [dict(zip(keys, values)) for values in itertools.product(*(grid[k] for k in keys))]
    checkpoints = sorted({int(v) for v in grid['iterations']})
    fits, where = [], []
    for e in entries:
        key = (float(e['learning_rate']), int(e['depth']), float(e['l2_leaf_reg']))
        if key not in fits:
            fits.append(key)
        where.append((fits.index(key), checkpoints.index(int(e['iterations']))))
    return entries, fits, where, checkpoints


def _philox4x32_10(idx, stream, seed):
    """Philox4x32-10 on the host, as csrc/pfn_device.h: counter (idx, stream) as two 64-bit halves, key = seed.  Returns four 32-bit words."""
    M = 0xFFFFFFFF
    c0, c1, c2, c3 = idx & M, (idx >> 32) & M, stream & M, (stream >> 32) & M
    k0, k1 = seed & M, (seed >> 32) & M
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & M, p1 & M, ((p0 >> 32) ^ c3 ^ k1) & M, p0 & M
        k0, k1 = (k0 + 0x9E3779B9) & M, (k1 + 0xBB67AE85) & M
    return c0, c1, c2, c3


def _catboost_holdout(y, seed, window):
    """CatBoost's grid_search as recalled: by default it does NOT cross-validate the candidates; it trains each on a shuffled stratified 80 % of
    the rows and scores it on the other 20 % by the loss function -- `cv=5` only feeds statistics the reference discards -- and refits the best on all rows.  The
    library's own shuffle is not restated: per class, floor(0.2 count + 0.5) rows are held out, at least 1 where the class has 2 or more, namely those of smallest
    (word, row index), row i's word being component i & 3 of philox4x32_10(i >> 2, stream = window, key = seed).  Returns fold [n] int32: 0 = held out, 1 = kept."""
    cls = np.asarray(y).reshape(-1) > 0.5
    words = np.array([_philox4x32_10(i >> 2, int(window), int(seed))[i & 3] for i in range(len(cls))], dtype=np.int64)
    fold = np.ones(len(cls), dtype=np.int32)
    for k in (False, True):
        idx = np.flatnonzero(cls == k)
        count = int(np.floor(CATBOOST_HOLDOUT * len(idx) + 0.5))
        if len(idx) >= 2:
            count = max(count, 1)
        fold[idx[np.lexsort((idx, words[idx]))[:count]]] = 0
    return fold


def _catboost_select(hold_margin, fold, cls, where, test_margin):
    """The host half of one problem's grid search, in f64: hold_margin [fits, NK, n] the margins of the search fits at every checkpoint, fold [n] (0 = held out),
    cls [n] bool, where = every entry's (fit, checkpoint), test_margin [fits, NK, T] of the refits.  An entry's score is the mean log loss of the held-out rows;
    a NaN (a fit that did not run or left the finite numbers) ranks last, the FIRST minimum wins.  Returns (log loss [entries] f64, best entry, proba [T] f64 =
    sigmoid(margin) of the best entry's refit at its checkpoint)."""
    hold_margin, cls = np.asarray(hold_margin, dtype=np.float64), np.asarray(cls, dtype=bool)
    held = np.asarray(fold) == 0
    z = np.where(cls[held], -1., 1.) * hold_margin[:, :, held]
    with np.errstate(invalid='ignore'):      # (a NaN margin is a NaN loss: it ranks last)
        per_fit = np.logaddexp(0., z).mean(-1) if held.any() else np.full(hold_margin.shape[:2], np.nan)
    loss = np.array([per_fit[c, k] for c, k in where], dtype=np.float64)
    best = int(np.argmin(np.where(np.isnan(loss), np.inf, loss)))
    c, k = where[best]
    return loss, best, 1. / (1. + np.exp(-np.asarray(test_margin, dtype=np.float64)[c, k]))


def _catboost_batched(x, y, test_x, test_y, return_params=False, seed=0, details=None):
    """CatBoost with the reference's grid search for W problems at once: x [n, W, F] normalised train rows, y [n, W], test_x [T, W, F], test_y [T, W] on the GPU.
    One pfn_catboost_cv launch grows the 70 trees of all W x 27 x 2 fits (the search fit on the kept 80 %, the refit on all rows) and writes their margins at 10,
    40 and 70 trees; the hold-out (before) and the 81 log losses and the selection (after) are host arithmetic.  Returns (ROC-AUC [W], proba [T, W]) numpy, and
    with return_params the chosen parameter dict of every problem as a third entry.  `details`, a dict, receives the launch's margins, status and trees, the
    folds and every problem's (log losses, best)."""
    n, W, F = x.shape
    entries, fits, where, checkpoints = _catboost_grid()
    depth = [d for _, d, _ in fits]
    hipops.catboost_cv_check(n, test_x.shape[0], F, depth, checkpoints[-1])
    if not x.is_cuda:
        raise NotImplementedError('catboost_metric runs on the GPU only (pfn_catboost_cv); there is no CPU path')
    cls = y.detach().cpu().numpy() > 0.5
    for w in range(W):
        if cls[:, w].all() or not cls[:, w].any():
            raise ValueError(f'catboost_metric: the train rows of window {w} hold one class only')
    folds = np.stack([_catboost_holdout(cls[:, w], seed, w) for w in range(W)])
    out = hipops.catboost_cv(x.float().transpose(0, 1).contiguous(), y.float().t().contiguous(), test_x.float().transpose(0, 1).contiguous(),
                             torch.from_numpy(folds).to(x.device), depth, [lr for lr, _, _ in fits], [l2 for _, _, l2 in fits], checkpoints[-1],
                             checkpoints=checkpoints, seed=seed, want_trees=details is not None)
    hold_margin, test_margin = out.hold_margin.double().cpu().numpy(), out.test_margin.double().cpu().numpy()
    chosen = [_catboost_select(hold_margin[w], folds[w], cls[:, w], where, test_margin[w]) for w in range(W)]
    if details is not None:
        details.update(hold_margin=hold_margin, test_margin=test_margin, status=out.status.cpu().numpy(), folds=folds,
                       trees=tuple(t.cpu().numpy() for t in out[3:]), scores=[(c[0], c[1]) for c in chosen])
    metric, proba = _fold_metric(chosen, test_y)
    return (metric, proba, [entries[c[1]] for c in chosen]) if return_params else (metric, proba)


@_single_problem(_catboost_batched)
def catboost_metric(x, y, test_x, test_y, categorical_feats):
    """Reference tabular.py:561-596 for one problem: x [n, F] (normalised) train rows, y [n], test_x [T, F], test_y [T] on the GPU -> (ROC-AUC, proba [T]) of the
    boosted symmetric trees (logistic loss, Cosine score, Newton leaves) that a grid search over the 81 entries of param_grid['catboost'] picks by the log loss on
    a stratified 20 % hold-out and refits on all rows.  categorical_feats is accepted and ignored: the reference casts those
    columns to int and never passes them as cat_features, so every column is numeric.  `catboost_metric.batched` is the same for many problems in one launch;
    `batch_pred` uses it."""
