"""Host-side checks of the BNN-classifier baseline (csrc/bnn_cv.hip, hipops.bnn_cv, tabular.bayes_net_metric): the C ABI and the build, the entry point's
argument checks, the restatement tests/bnn_cv_f64.py against autograd, central differences and torch.optim.Adam, the rank-one form the kernel uses against the
dense one, the noise addressing, the grid against scikit-learn, the host half of the grid search, the recorded fixture, and the kernel's compiled budgets.  No GPU."""
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bnn_cv_f64 as cvf      # noqa: E402
import bnn_f64 as ref      # noqa: E402
import tabular_cases      # noqa: E402

from transformerscandobayesianinference_amd import _hip, hipops, tabular      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'transformerscandobayesianinference_amd', 'csrc')
PFN_ERR_UNSUPPORTED, PFN_ERR_ARGUMENT = -1, -4


def small_fit(n=12, F=3, H=5, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, F, generator=g)
    y = (torch.rand(n, generator=g) > 0.5).float()
    D = ref.num_params(F, H)
    loc, u = torch.randn(D, generator=g).double(), (torch.randn(D, generator=g) * 0.5 - 1.).double()
    mask = np.arange(n) % 3 != 1
    return x, y, mask, loc, u, D


def test_the_symbol_is_declared_exported_and_bound_at_abi_10():
    header = open(os.path.join(ROOT, 'include', 'pfn_hip.h')).read()
    source = open(os.path.join(CSRC, 'bnn_cv.hip')).read()
    lib = _hip.lib()
    assert re.search(r'\bpfn_bnn_cv\s*\(', header)
    assert 'pfn_bnn_cv' in _hip.SIGNATURES and hasattr(lib, 'pfn_bnn_cv') and len(_hip.SIGNATURES['pfn_bnn_cv'][1]) == 29
    assert re.search(r'^extern "C" int pfn_bnn_cv\s*\(', source, re.M) and re.search(r'\blaunch_bnn_cv\s*\(', source) and 'struct BnnCvArgs' in source
    assert _hip.ABI_VERSION == 10 and lib.pfn_abi_version() == 10 and '#define PFN_ABI_VERSION 10' in header
    for name, value in (('FOLDS', 5), ('SLOTS', 6), ('MAX_CANDIDATES', 64), ('UNUSED', 0), ('DONE', 1), ('NONFINITE', 2)):
        assert f'#define PFN_BNN_CV_{name} {value}\n' in header and getattr(hipops, 'BNN_CV_' + name) == value, name
    assert (cvf.SLOTS, cvf.FOLDS, cvf.UNUSED, cvf.DONE, cvf.NONFINITE) == (6, 5, 0, 1, 2)
    assert callable(hipops.bnn_cv) and callable(hipops.bnn_cv_check) and callable(hipops.bnn_cv_state)
    assert callable(tabular.bayes_net_metric) and tabular.bayes_net_metric.batched is tabular._bayes_batched
    build = open(os.path.join(CSRC, 'build.sh')).read()
    assert 'bnn_cv.hip' in build and '../_build/bnn_cv.o' in build      # compiled and linked
    for shared in ('bnn_adam', 'bnn_sigmoid', 'philox4x32_10', 'normal4', 'launch_lds', 'fold_shapes'):
        assert re.search(r'\b%s\s*\(' % shared, source), shared      # the shared pieces, not copies of them
    assert 'stay out: they need libraries' in tabular.__doc__ and 'BNN classifier, whose grid cannot run' not in tabular.__doc__


def test_argument_errors_return_before_any_launch():
    lib = _hip.lib()
    buf = torch.zeros(4096)      # host memory standing in for device buffers: a refused call never looks at it
    p = buf.data_ptr()
    H_ok, lr_ok = np.array([5, 64], dtype=np.int32), np.array([1e-3, 1e-4], dtype=np.float32)

    def call(P=1, n=8, T=2, F=3, NC=2, n_splits=4, H=H_ok, lr=lr_ok, ld=64 * 6 + 2, step0=0, num_steps=3, b1=0.9, b2=0.999, eps=1e-8, S=2, train=p, state=p, status=p,
             cv_prob=p, test_prob=p, cand_null=False):
        return lib.pfn_bnn_cv(train, p, p, p, 0 if cand_null else H.ctypes.data, lr.ctypes.data, P, n, T, F, NC, n_splits, state, ld, step0, num_steps, b1, b2, eps, S, 7,
                              0, 0, cv_prob, test_prob, 0, 0, status, 0)
    i32, f32 = (lambda *v: np.array(v, dtype=np.int32)), (lambda *v: np.array(v, dtype=np.float32))
    for kw in (dict(n=3), dict(n=129), dict(T=0), dict(T=129), dict(F=0), dict(F=129), dict(NC=0), dict(NC=65), dict(H=i32(5, 0)), dict(H=i32(65, 5))):
        assert call(**kw) == PFN_ERR_UNSUPPORTED, kw
    assert call(n=3) == PFN_ERR_UNSUPPORTED and b'4 .. 128' in lib.pfn_last_error_string()
    for kw in (dict(P=0), dict(n_splits=1), dict(n_splits=6), dict(train=0), dict(state=0), dict(status=0), dict(cand_null=True), dict(ld=64 * 6 + 1), dict(step0=-1),
               dict(step0=(1 << 40) + 1), dict(num_steps=-1), dict(S=-1), dict(S=(1 << 20) + 1), dict(lr=f32(1e-3, -1.)), dict(lr=f32(float('nan'), 1.)),
               dict(lr=f32(float('inf'), 1.)), dict(b1=1.), dict(b1=-0.1), dict(b2=1.), dict(eps=-1.), dict(cv_prob=0), dict(test_prob=0)):
        assert call(**kw) == PFN_ERR_ARGUMENT, kw
    # the limits first, before the arguments and before any pointer is looked at
    assert call(n=3, train=0, P=0) == PFN_ERR_UNSUPPORTED and call(H=i32(5, 65), P=0, state=0) == PFN_ERR_UNSUPPORTED
    assert call(S=0, cv_prob=0, test_prob=0, P=0) == PFN_ERR_ARGUMENT
    # nothing to do: returns at once (the host stand-ins would fault a launch)
    assert call(num_steps=0, S=0) == 0 and call(num_steps=0, S=0, cv_prob=0, test_prob=0) == 0


def test_python_checks_raise_before_the_device_is_asked_for():
    fold = torch.zeros(1, 8, dtype=torch.int32)
    x, y, tx = torch.zeros(1, 8, 3), torch.zeros(1, 8), torch.zeros(1, 2, 3)
    with pytest.raises(ValueError, match='n = 3'):
        hipops.bnn_cv_check(3, 2, 3, [5])
    with pytest.raises(ValueError, match='H = 65'):
        hipops.bnn_cv_check(8, 2, 3, [5, 65])
    with pytest.raises(ValueError, match='NC = 65'):
        hipops.bnn_cv_check(8, 2, 3, [5] * 65)
    state = hipops.bnn_cv_state(1, [5, 10], 3, 'cpu')
    assert state.shape == (1, 2, 6, 6, 62) and float(state[0, 1, 2, 1, 3]) == pytest.approx(math.log(math.expm1(0.1))) and not state[:, :, :, (0, 2, 3, 4, 5)].any()
    with pytest.raises(ValueError, match='F = 129'):
        hipops.bnn_cv(torch.zeros(1, 8, 129), y, torch.zeros(1, 2, 129), fold, 4, [5], [1e-3], state, 1)
    with pytest.raises(ValueError):
        hipops.bnn_cv(x, y, tx, fold, 4, [5, 10], [1e-3, -1.], state, 1)
    with pytest.raises(ValueError):
        hipops.bnn_cv(x, y, tx, fold, 6, [5, 10], [1e-3, 1e-3], state, 1)
    with pytest.raises(ValueError, match='F = 129'):
        tabular.bayes_net_metric(torch.zeros(8, 129), torch.zeros(8), torch.zeros(2, 129), torch.zeros(2), [])
    # with sound arguments the product path asks for the GPU: there is no CPU fall-back
    with pytest.raises(_hip.HipExtensionError):
        hipops.bnn_cv(x, y, tx, fold, 4, [5, 10], [1e-3, 1e-3], state, 1)
    with pytest.raises(NotImplementedError):
        tabular.bayes_net_metric(torch.randn(8, 3), torch.tensor([0., 1.] * 4), torch.randn(2, 3), torch.zeros(2), [])


def test_restated_gradient_against_autograd_and_central_differences():
    x, y, mask, loc, u, D = small_fit()
    F, H = 3, 5
    eps = cvf.step_noise(3, cvf.stream(2, 1), 0, D)
    a, b = loc.clone().requires_grad_(True), u.clone().requires_grad_(True)
    L = cvf.loss(a, b, eps, x, y, mask, F, H)
    ga, gb = torch.autograd.grad(L, (a, b))
    L = L.detach()
    for grads in (cvf.dense_grads, cvf.rank_one_grads):
        L2, g_loc, g_u = cvf.loss_and_grads(loc, u, eps, x, y, mask, F, H, grads=grads)
        assert abs(float(L2) - float(L)) <= 1e-12 * abs(float(L))
        assert float((g_loc - ga).norm() / ga.norm()) <= 1e-12 and float((g_u - gb).norm() / gb.norm()) <= 1e-12
    h = 1e-6
    for i in (0, 7, H * F, H * F + H + 1, H * F + 2 * H + 3, D - 2, D - 1):
        e = torch.zeros(D, dtype=torch.float64)
        e[i] = h
        fd_loc = (cvf.loss(loc + e, u, eps, x, y, mask, F, H) - cvf.loss(loc - e, u, eps, x, y, mask, F, H)) / (2 * h)
        fd_u = (cvf.loss(loc, u + e, eps, x, y, mask, F, H) - cvf.loss(loc, u - e, eps, x, y, mask, F, H)) / (2 * h)
        assert abs(float(fd_loc) - float(g_loc[i])) <= 1e-7 * max(1., abs(float(g_loc[i]))) and abs(float(fd_u) - float(g_u[i])) <= 1e-7 * max(1., abs(float(g_u[i])))
    # a masked row takes no part, whatever it holds
    x2 = x.clone()
    x2[~torch.as_tensor(mask)] = float('nan')
    assert torch.equal(cvf.loss_and_grads(loc, u, eps, x2, y, mask, F, H)[1], cvf.loss_and_grads(loc, u, eps, x, y, mask, F, H)[1])


@pytest.mark.parametrize('n,F,H', [(12, 3, 5), (40, 60, 30), (128, 128, 64)])
def test_the_rank_one_form_equals_the_dense_one_in_f64(n, F, H):
    x, y, mask, loc, u, D = small_fit(n, F, H, seed=n)
    theta = loc + cvf.softplus(u) * cvf.step_noise(1, 0, 5, D)
    (U1, g1), (U2, g2) = cvf.dense_grads(theta, x, y, mask, F, H), cvf.rank_one_grads(theta, x, y, mask, F, H)
    assert abs(float(U1 - U2)) <= 1e-12 * abs(float(U1)) and float((g1 - g2).norm() / g1.norm()) <= 1e-12
    assert abs(float(U1 - cvf.potential(theta, x, y, mask, F, H))) <= 1e-12 * abs(float(U1))      # bnn_f64.potentials on the compacted rows


def test_ten_steps_against_torch_adam():
    x, y, mask, loc, u, D = small_fit()
    F, H, lr, q, seed = 3, 5, 0.05, cvf.stream(1, 2), 9
    state = torch.zeros(6, D, dtype=torch.float64)
    state[0], state[1] = loc, u
    after, losses = cvf.run(state, x, y, mask, F, H, lr, q, seed, 0, 10)
    a, b = loc.clone().requires_grad_(True), u.clone().requires_grad_(True)
    opt = torch.optim.Adam([a, b], lr=ref.f32(lr), betas=(ref.f32(0.9), ref.f32(0.999)), eps=ref.f32(1e-8))
    for t in range(10):
        opt.zero_grad()
        L = cvf.loss(a, b, cvf.step_noise(seed, q, t, D), x, y, mask, F, H)
        assert abs(float(L.detach()) - losses[t]) <= 1e-10 * abs(losses[t])
        L.backward()
        opt.step()
    assert float((after[0] - a.detach()).norm() / a.detach().norm()) <= 1e-10 and float((after[1] - b.detach()).norm() / b.detach().norm()) <= 1e-10
    # a split run is the unsplit one
    mid, _ = cvf.run(state, x, y, mask, F, H, lr, q, seed, 0, 4)
    assert torch.equal(cvf.run(mid, x, y, mask, F, H, lr, q, seed, 4, 6)[0], after)


def test_noise_addressing():
    D = ref.num_params(128, 64)
    assert D == 8386 and (D - 1) >> 2 == 2096 < 4096
    step_hi = cvf.block_index((1 << 40) + (1 << 31), D)      # the last step a call can reach
    pred_lo, pred_hi = cvf.block_index(cvf.PRED_DOMAIN, D), cvf.block_index(cvf.PRED_DOMAIN + (1 << 20), D)
    obs_lo = cvf.block_index(cvf.OBS_DOMAIN, 256)
    assert int(cvf.block_index(0, D)[-1]) == 2096 and int(step_hi[-1]) < int(pred_lo[0]) and int(pred_hi[-1]) < int(obs_lo[0])
    assert int(cvf.block_index(cvf.OBS_DOMAIN + (1 << 20), 256)[-1]) < 1 << 64
    assert int(cvf.block_index(5, 9)[2]) == (5 << 12) | 2 and len(cvf.block_index(5, 9)) == 3
    # component i & 3 of block i >> 2, from the scalar Philox of tests/nuts_f64.py
    import nuts_f64 as emu
    z = cvf.step_noise(11, cvf.stream(3, 2), 6, 9)
    for i in (0, 3, 5, 8):
        assert abs(float(z[i]) - emu.normal4(emu.philox4x32_10((6 << 12) | (i >> 2), 26, 11))[i & 3]) <= 1e-15
    z = cvf.pred_noise(11, 26, 4, 9)
    assert abs(float(z[6]) - emu.normal4(emu.philox4x32_10(((cvf.PRED_DOMAIN + 4) << 12) | 1, 26, 11))[2]) <= 1e-15
    un = cvf.obs_uniforms(11, 26, 4, 7)
    assert float(un[6]) == emu.u01(emu.philox4x32_10(((cvf.OBS_DOMAIN + 4) << 12) | 1, 26, 11)[2]) and bool(((un >= 0) & (un < 1)).all())
    assert cvf.stream(3, 2) == 26      # q: the candidate takes no part
    z32 = cvf.step_noise(11, 26, 6, 4000, torch.float32)
    assert z32.dtype == torch.float32 and float((z32.double() - cvf.step_noise(11, 26, 6, 4000)).abs().max()) < 1e-5


def test_grid_enumeration_is_parametergrids_and_the_references_grid_search_raises():
    reference = {'embed': [5, 10, 30, 64], 'lr': [1e-3, 1e-4], 'num_training_steps': [400], 'num_samples_for_prediction': [400]}
    assert tabular.param_grid['bayes'] == reference == cvf.PARAM_GRID
    entries, cands, num_steps, num_draws = tabular._bayes_grid()
    assert cands == [(5, 1e-3), (5, 1e-4), (10, 1e-3), (10, 1e-4), (30, 1e-3), (30, 1e-4), (64, 1e-3), (64, 1e-4)] and (num_steps, num_draws) == (400, 400)
    assert entries == cvf.grid_entries()
    with pytest.raises(ValueError):
        tabular._bayes_grid(dict(reference, num_training_steps=[400, 800]))
    model_selection = pytest.importorskip('sklearn.model_selection')
    base = pytest.importorskip('sklearn.base')
    assert entries == list(model_selection.ParameterGrid(reference))

    class WithTheReferencesConstructor(base.BaseEstimator, base.ClassifierMixin):      # reference tabular.py:416: (num_features, n_layers, embed, lr, device)
        def __init__(self, num_features, n_layers, embed, lr, device):
            self.num_features, self.n_layers, self.embed, self.lr, self.device = num_features, n_layers, embed, lr, device

        def fit(self, X, y):
            self.classes_ = np.unique(y)
            return self

        def predict(self, X):
            return np.zeros(len(X))
    X, y = np.random.RandomState(0).randn(20, 3), np.arange(20) % 2
    with pytest.raises(ValueError, match='num_samples_for_prediction|num_training_steps'):      # the deviation INTEGRATION.md records: the reference's grid cannot run
        model_selection.GridSearchCV(WithTheReferencesConstructor(3, 2, 5, 1e-3, 'cpu'), reference, cv=5).fit(X, y)


def test_selection_on_hand_made_probabilities():
    folds = np.array([0, 0, 1, 1, 0, 1], dtype=np.int32)
    cls = np.array([1, 0, 1, 0, 1, 0], dtype=bool)
    cv_prob = np.array([[0.9, 0.1, 0.5, 0.2, 0.4, 0.7],      # fold 0: 2 of 3, fold 1: (0.5 predicts class 0: wrong), right, wrong: 1 of 3 -> 1/2
                        [0.6, 0.4, 0.6, 0.4, 0.6, 0.6],      # 3 of 3, 2 of 3 -> 5/6
                        [0.51, 0.49, 0.9, 0.1, 0.8, 0.9],    # the same score later: the first wins
                        [0.5, 0.5, 0.5, 0.5, 0.5, 0.5]])     # everything predicts class 0: 1 of 3, 2 of 3 -> 1/2
    test_prob = np.arange(8.).reshape(4, 2) / 10
    mean, best, proba = tabular._bayes_select(cv_prob, folds, cls, 2, test_prob)
    assert mean.dtype == np.float64 and mean.tolist() == [0.5, (1. + 2 / 3) / 2, (1. + 2 / 3) / 2, 0.5] and best == 1 and proba.tolist() == [0.2, 0.3]
    mean2, best2 = cvf.select(cv_prob, folds, cls, 2)
    assert mean2.tobytes() == mean.tobytes() and best2 == best
    cv_prob[1, 0] = np.nan      # a fit that left the finite numbers ranks last
    mean, best, _ = tabular._bayes_select(cv_prob, folds, cls, 2, test_prob)
    assert np.isnan(mean[1]) and best == 2


def test_the_start_of_a_fit_depends_on_seed_problem_and_candidate_alone():
    a = tabular._bayes_loc0(3, 2, 1, 317)
    assert a.shape == (6, 317) and a.dtype == torch.float32 and torch.equal(a, tabular._bayes_loc0(3, 2, 1, 317))
    assert not torch.equal(a, tabular._bayes_loc0(3, 2, 0, 317)) and not torch.equal(a, tabular._bayes_loc0(3, 1, 1, 317)) and not torch.equal(a, tabular._bayes_loc0(4, 2, 1, 317))
    assert 0.25 < float(a.std()) < 0.4      # the median of 15 standard normals: std about 0.32


def test_the_recorded_fixture_is_what_the_generators_still_draw():
    rec = torch.load(os.path.join(ROOT, 'tests', 'golden', 'tabular_bnn.pt'), weights_only=False)
    assert rec['cands'] == tabular._bayes_grid()[1] and (rec['num_steps'], rec['num_draws']) == (400, 400) and len(rec['problems']) == len(cvf.SHAPES)
    clean = 0
    for r, (n, F, T) in zip(rec['problems'], cvf.SHAPES):
        x, y, tx, ty = tabular_cases.problem(n, F, T, r['seed'])
        assert x.shape == (n, F) and tx.shape == (T, F) and r['checksum'] == float(np.float64(x).sum() + np.float64(tx).sum() + y.sum())
        folds = tabular._stratified_folds(y > 0.5, r['n_splits'])
        assert r['n_splits'] == min(5, n // 2) and np.array_equal(folds, r['folds'].numpy())
        cv_prob, test_prob = r['cv_prob'].numpy(), r['test_prob'].numpy()
        assert cv_prob.shape == (8, n) and test_prob.shape == (8, T) and cv_prob.dtype == np.float64 and np.isfinite(cv_prob).all() and np.isfinite(test_prob).all()
        mean, best, proba = tabular._bayes_select(cv_prob, folds, y > 0.5, r['n_splits'], test_prob)
        assert mean.tobytes() == r['mean_test_score'].numpy().tobytes() and best == r['best'] and np.array_equal(proba, test_prob[best])
        # the windows the seeds were chosen for, on the f64 results alone
        window = 4 * max(r['e'], 2. ** -23)
        near = np.abs(cv_prob - 0.5) <= window
        assert near.mean() <= 0.02 and int(near.sum()) == r['near_half']
        clean += int(not near.any())
        assert 0 < r['e'] < 1e-3
    assert clean >= 3


def test_the_kernel_keeps_its_register_scratch_and_lds_budgets(tmp_path):
    import shutil
    import subprocess
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    asm = str(tmp_path / 'bnn_cv.s')
    subprocess.run([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-munsafe-fp-atomics', '-Wno-unused-result', '-S', '--cuda-device-only',
                    os.path.join(CSRC, 'bnn_cv.hip'), '-o', asm], check=True, capture_output=True)
    found = re.findall(r'\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel', open(asm).read(), re.S)
    assert len(found) == 1 and 'bnn_cv_kernel' in found[0][0]      # one kernel for every width: the candidates of a call share a launch
    body = found[0][1]
    static_lds = int(re.search(r'\.amdhsa_group_segment_fixed_size (\d+)', body).group(1))
    assert int(re.search(r'\.amdhsa_private_segment_fixed_size (\d+)', body).group(1)) == 0      # no scratch
    assert int(re.search(r'\.amdhsa_next_free_vgpr (\d+)', body).group(1)) <= 128      # four waves per SIMD
    assert static_lds <= 512

    def lds_bytes(n, T, F, H):      # bnn_cv_lds_bytes
        Dp = (H * (F + 3) + 2 + 3) & ~3
        return 4 * (16 + max(n, T) * (F | 1) + 2 * Dp + 2 * H + 2 * F + 2 * n + 4)
    assert lds_bytes(128, 128, 128, 64) == 135792 and lds_bytes(128, 128, 128, 64) + static_lds <= 160 * 1024
    assert lds_bytes(80, 20, 60, 64) == 53520 and 3 * (lds_bytes(80, 20, 60, 64) + static_lds) <= 160 * 1024      # the study's shape: three blocks share a CU
    text = open(os.path.join(CSRC, 'bnn_cv.hip')).read()
    assert '(16 + (size_t)(n > T ? n : T) * (F | 1) + 2 * Dp + 2 * (size_t)H + 2 * (size_t)F + 2 * (size_t)n + 4) * 4' in text and 'static_assert' in text
