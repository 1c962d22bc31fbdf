"""The tabular study's evaluation protocol: the batched device paths against what they replace, on the same table, model and GPU.

    python tools/bench_tabular.py [--precision fp16] [--out profiles/r16_tabular.json]

bptt 100, eval positions 10 / 20 / 40 / 80, 20 windows of a 60-feature table, a PFN of the configs[3] size (emsize 512, 4 heads, nhid 1024, 6 layers, BCE head):
pfn_batched   tabular.evaluate_position(model): one pfn_tabular_windows launch, ONE forward at batch 20 T, one pfn_auc_counts launch, results on the host
pfn_looped    the reference's form of the same work (tabular.py:288-301): T times (torch's normalisation, model(...) at batch 20, sigmoid, .cpu()), then the metric
knn_batched   tabular.evaluate_position(knn_metric): one TRAIN_ONLY window launch and one pfn_knn_cv launch for all 20 windows; reported per window
knn_sklearn   per window: GridSearchCV(KNeighborsClassifier(), k = 1 .. 5, cv = 5) + predict_proba + roc_auc_score on the host (needs scikit-learn)

Protocol: wall-clock time of whole calls, host work and transfers included (that is what a user waits for), the device synchronised at both ends; every variant
is warmed up, the variants alternate, REPS rounds; the figure is the median round, the spread (max - min) / median.  Needs a GPU."""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from transformerscandobayesianinference_amd import encoders, tabular  # noqa: E402
from transformerscandobayesianinference_amd.transformer import TransformerModel  # noqa: E402

REPS = 7
BPTT, WINDOWS, FEATURES = 100, 20, 60
POSITIONS = (10, 20, 40, 80)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--precision', default='fp16')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_tabular: no GPU -- nothing is measured without one')
    dev = 'cuda:0'
    torch.manual_seed(0)
    model = TransformerModel(encoders.Linear(FEATURES, 512), 1, 512, 4, 1024, 6, 0.0, y_encoder=encoders.Linear(1, 512), precision=a.precision)
    with torch.no_grad():
        for layer in model.transformer_encoder.layers:
            for t in (layer.linear2.weight, layer.self_attn.out_proj.weight):
                t.normal_(0, 0.02)
    model = model.to(dev).eval()
    g = torch.Generator().manual_seed(1)
    N = BPTT + 3 * WINDOWS
    X = (torch.randn(N, FEATURES, generator=g) * (0.5 + torch.rand(FEATURES, generator=g)) + torch.randn(FEATURES, generator=g)).to(dev)
    w = torch.randn(FEATURES, generator=g).to(dev)
    y = ((X - X.mean(0)) @ w + torch.randn(N, generator=g).to(dev) > 0).float()
    starts = tabular.select_windows(N, BPTT, WINDOWS).tolist()
    eval_xs = torch.stack([X[s:s + BPTT] for s in starts], 1)
    eval_ys = torch.stack([y[s:s + BPTT] for s in starts], 1)
    try:
        from sklearn import neighbors
        from sklearn.metrics import roc_auc_score
        from sklearn.model_selection import GridSearchCV
    except ImportError:
        neighbors = None
    res = dict(bptt=BPTT, windows=WINDOWS, features=FEATURES, model='emsize 512, 4 heads, nhid 1024, 6 layers, 1 output', precision=a.precision, reps=REPS,
               device=torch.cuda.get_device_name(0), positions={})
    for sep in POSITIONS:
        T = BPTT - sep
        keep = {}

        def pfn_batched():
            keep['batched'] = tabular.evaluate_position(X, y, [], model, BPTT, sep, max_samples=WINDOWS)

        def pfn_looped():
            outputs = np.zeros((T, WINDOWS))
            with torch.no_grad():
                for i, pos in enumerate(range(sep, BPTT)):
                    eval_x = torch.cat([eval_xs[:sep], eval_xs[pos].unsqueeze(0)])
                    eval_x = (eval_x - eval_x.mean(0)) / (eval_x.std(0) + .000001)
                    outputs[i] = torch.sigmoid(model((eval_x, eval_ys[:sep]), single_eval_pos=sep)).squeeze(-1).squeeze(0).cpu().numpy()
            keep['looped'] = (tabular.roc_auc_columns(torch.from_numpy(outputs).float().to(dev), eval_ys[sep:])[0], outputs)

        def knn_batched():
            keep['knn'] = tabular.evaluate_position(X, y, [], tabular.knn_metric, BPTT, sep, max_samples=WINDOWS)

        def knn_sklearn():
            out = []
            for wi in range(WINDOWS):
                ex = eval_xs[:, wi]
                ex = ((ex - ex[:sep].mean(0)) / (ex[:sep].std(0) + .000001)).cpu()
                ey = eval_ys[:, wi].cpu()
                clf = GridSearchCV(neighbors.KNeighborsClassifier(), {'n_neighbors': np.arange(1, min(6, sep - 1))}, cv=min(5, sep // 2))
                clf.fit(ex[:sep], ey[:sep].long())
                pred = clf.predict_proba(ex[sep:])[:, 1]
                out.append((roc_auc_score(ey[sep:].numpy(), pred) if 0 < ey[sep:].sum() < T else float('nan'), pred))
            keep['sklearn'] = out

        variants = dict(pfn_batched=pfn_batched, pfn_looped=pfn_looped, knn_batched=knn_batched)
        if neighbors is not None:
            variants['knn_sklearn'] = knn_sklearn
        times = {name: [] for name in variants}
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            for fn in variants.values():
                fn()
            for _ in range(REPS):
                for name, fn in variants.items():
                    times[name].append(wall(fn))
        pos = dict(test_rows_per_window=T, variants={})
        for name, ts in times.items():
            med = statistics.median(ts)
            pos['variants'][name] = dict(median_ms=med * 1e3, min_ms=min(ts) * 1e3, max_ms=max(ts) * 1e3, spread=(max(ts) - min(ts)) / med)
        V = pos['variants']
        pos['pfn_speedup'] = V['pfn_looped']['median_ms'] / V['pfn_batched']['median_ms']
        pos['pfn_faster_beyond_spread'] = V['pfn_batched']['max_ms'] < V['pfn_looped']['min_ms']
        pos['knn_ms_per_window'] = V['knn_batched']['median_ms'] / WINDOWS
        # the paths agree on what they both compute
        pos['pfn_outputs_max_abs_batched_vs_looped'] = float(np.abs(keep['batched'][1] - keep['looped'][1]).max())
        if neighbors is not None:
            pos['knn_sklearn_ms_per_window'] = V['knn_sklearn']['median_ms'] / WINDOWS
            pos['knn_speedup_per_window'] = V['knn_sklearn']['median_ms'] / V['knn_batched']['median_ms']
            pos['knn_windows_with_sklearns_proba'] = int(sum(np.array_equal(keep['knn'][1][:, wi], keep['sklearn'][wi][1]) for wi in range(WINDOWS)))
        res['positions'][str(sep)] = pos
    print(json.dumps(res, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or '.', exist_ok=True)
        json.dump(res, open(a.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
