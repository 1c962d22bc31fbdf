"""Seeded inputs shared by the CatBoost-baseline tests (tests/test_host_catboost.py, tests/test_gpu_catboost.py) and tools/record_catboost_cv_fixtures.py: the
shape matrix of the kernel test with its planted columns, the synthetic problems and the windows of the diabetes table whose f64 fits and grid searches
tests/golden/tabular_catboost.pt records, and the planted faults of the sensitivity study.  Everything is drawn on the CPU from numpy's RandomState, so the
recorder and the tests see the same numbers."""
import numpy as np

import tabular_cases
from xgb_cases import GRID_WINDOWS, diabetes_window      # noqa: F401  (the same two windows of tests/golden/tabular_diabetes.pt as the gradient-boosting tests)

# label -> (n, F, T, [(depth, learning_rate, l2)], trees, checkpoints, slots followed on the host).
# Together: n of {10, 63, 64, 65, 128} (one half-wave, the 64-position boundary from both sides, both halves full), F of {1, 5, 60, 128}, T of {1, 128},
# depth of {1, 2, 4, 7}, l2 of {0, 0.5, 1}, trees of {1, 3, 20}.  Both slots of every case run on the device; the larger cases follow one slot to stay quick.
BOTH = (0, 1)
CASES = {
    'n10_F1_T1': (10, 1, 1, [(1, 0.5, 0.5), (2, 0.1, 1.0)], 3, (1, 3), BOTH),
    'n10_F5_T128': (10, 5, 128, [(4, 0.5, 0.0), (7, 0.1, 0.5)], 20, (1, 3, 20), BOTH),
    'n63_F5_T1': (63, 5, 1, [(2, 1.0, 1.0), (7, 0.5, 0.0)], 3, (1, 3), BOTH),
    'n63_F60_T128': (63, 60, 128, [(4, 0.5, 0.5)], 3, (3,), (1,)),
    'n64_F1_T128': (64, 1, 128, [(7, 0.5, 1.0), (1, 1.0, 0.0)], 20, (10, 20), BOTH),
    'n64_F128_T1': (64, 128, 1, [(2, 0.1, 0.5)], 1, (1,), (0,)),
    'n65_F5_T128': (65, 5, 128, [(7, 0.1, 0.0), (4, 1.0, 1.0)], 3, (1, 3), BOTH),
    'n65_F60_T1': (65, 60, 1, [(1, 0.5, 0.5), (7, 0.5, 1.0)], 1, (1,), (0,)),
    'n65_F128_T1': (65, 128, 1, [(4, 0.5, 1.0)], 3, (2, 3), (1,)),
    'n128_F1_T1': (128, 1, 1, [(7, 0.5, 0.5), (2, 0.1, 0.0)], 20, (1, 20), BOTH),
    'n128_F5_T128': (128, 5, 128, [(7, 0.5, 1.0)], 20, (1, 3, 20), (1,)),
    'n128_F128_T128': (128, 128, 128, [(7, 0.5, 0.5), (2, 1.0, 0.0)], 1, (1,), (0,)),
}
assert {c[0] for c in CASES.values()} == {10, 63, 64, 65, 128} and {c[1] for c in CASES.values()} == {1, 5, 60, 128} and {c[2] for c in CASES.values()} == {1, 128}
assert {c[4] for c in CASES.values()} == {1, 3, 20} and {k[0] for c in CASES.values() for k in c[3]} == {1, 2, 4, 7}
assert {k[2] for c in CASES.values() for k in c[3]} == {0.0, 0.5, 1.0}
CASE_SEED, FIT_SEED = 900, 11
DUPLICATE, CONSTANT, THREE_VALUED = (0, 3), 1, 2      # from F = 5 on: column 3 repeats column 0, column 1 is constant, column 2 holds three values


def holdout_fold(y):
    """fold [n] int32 for the kernel tests (dealt here, not by tabular): in each class every fifth row, from the class's first, is held out (fold 0)."""
    fold = np.ones(len(y), dtype=np.int32)
    for k in (False, True):
        idx = np.flatnonzero((np.asarray(y) > 0.5) == k)
        fold[idx[::5]] = 0 if len(idx) > 1 else 1
    return fold


def case_problem(label, p=0):
    """Problem p of a case: float32 x [n,F], y [n], test_x [T,F], test_y [T] and fold [n] int32.  From F = 5 on the planted columns above."""
    n, F, T = CASES[label][:3]
    x, y, tx, ty = tabular_cases.problem(n, F, T, CASE_SEED + 17 * sorted(CASES).index(label) + p)
    x, tx = x.copy(), tx.copy()
    if F >= 5:
        both = np.concatenate([x, tx])
        both[:, THREE_VALUED] = np.sign(np.round(both[:, THREE_VALUED]))
        both[:, DUPLICATE[1]] = both[:, DUPLICATE[0]]
        both[:, CONSTANT] = 0
        x, tx = both[:n], both[n:]
    return x, y, tx, ty, holdout_fold(y)


def three_value_problem():
    """F = 1 with three distinct values: two borders, so a depth-4 tree must end after two levels."""
    rs = np.random.RandomState(CASE_SEED + 1000)
    x = rs.randint(-1, 2, size=(12, 1)).astype(np.float32)
    x[:3, 0] = (-1, 0, 1)
    y = ((x[:, 0] + 0.8 * rs.randn(12)) > 0).astype(np.float32)
    y[:2] = (0, 1)
    tx = np.array([[-1.], [0.], [1.], [0.5]], dtype=np.float32)
    return x, y, tx, np.zeros(4, dtype=np.float32), np.ones(12, dtype=np.int32)


def one_class_problem():
    """A hold-out that leaves a single class to learn on: the only rows of class 1 are held out.  Slot 0 must say ONE_CLASS, slot 1 fits."""
    x, y, tx, ty = tabular_cases.problem(10, 5, 4, CASE_SEED + 2000)
    y = np.zeros(10, dtype=np.float32)
    y[[2, 7]] = 1
    fold = np.ones(10, dtype=np.int32)
    fold[[2, 7]] = 0
    return x, y, tx, ty, fold


# the synthetic problems whose fits tests/golden/tabular_catboost.pt records for the structural comparison: (n, F, T, problem seed, trees)
STRUCTURAL = [(24, 5, 6, 1, 20), (40, 8, 10, 2, 20), (80, 20, 20, 3, 3), (65, 8, 5, 4, 3)]
STRUCTURAL_CANDS = [(2, 0.5, 0.5), (4, 0.1, 1.0), (7, 0.5, 0.0)]
# a level's best noisy score stands clear of the second by this share of |score| + |noise|: an f32 sum of up to 256 terms and a quotient are off by some
# 2^-24 * sqrt(256) = 1e-6 of the scale, and 1e-4 leaves two orders of magnitude
MIN_GAP = 1e-4

FAULTS = ('l2_dropped_from_score', 'noise_dropped', 'hessian_weights', 'border_between_equal', 'leaf_not_scaled', 'checkpoint_off_by_one', 'used_kept')
