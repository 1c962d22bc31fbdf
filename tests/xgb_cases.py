"""Seeded inputs shared by the gradient-boosting tests (tests/test_host_xgb.py, tests/test_gpu_xgb.py) and tools/record_xgb_cv_fixtures.py: the shape matrix of
the kernel test with its planted columns, the synthetic problems and the windows of the diabetes table whose f64 grid searches tests/golden/tabular_xgb.pt
records, and the planted faults of the sensitivity study.  Everything is drawn on the CPU from numpy's RandomState, so the recorder and the tests see the same
numbers."""
import numpy as np

import tabular_cases

# label -> (n, F, T, [(max_depth, learning_rate, min_child_weight, subsample, colsample)], rounds, slots checked against the restatement).
# Together: n of {10, 63, 64, 65, 128} (one half-wave, the 64-position boundary from both sides, both halves full), F of {1, 5, 60, 128}, T of {1, 128},
# depth 1 and 2, rounds 1, 3 and 20.  Every slot of every case runs on the device; the larger cases follow two slots on the host to stay quick.
ALL = (0, 1, 2, 3, 4, 5)
CASES = {
    'n10_F1_T1': (10, 1, 1, [(1, 0.2, 0.5, 0.8, 0.8), (2, 0.02, 0.25, 1.0, 1.0)], 3, ALL),
    'n10_F5_T128': (10, 5, 128, [(2, 0.2, 0.25, 0.8, 0.8), (1, 0.2, 0.5, 0.5, 0.5)], 20, ALL),
    'n63_F5_T1': (63, 5, 1, [(2, 0.2, 1.0, 0.8, 0.8), (1, 0.02, 0.5, 0.5, 0.8)], 3, ALL),
    'n63_F60_T128': (63, 60, 128, [(2, 0.2, 0.5, 0.8, 0.8)], 3, (1, 5)),
    'n64_F1_T128': (64, 1, 128, [(2, 0.2, 1.0, 0.5, 0.8), (1, 0.2, 0.5, 1.0, 1.0)], 20, (0, 5)),
    'n64_F128_T1': (64, 128, 1, [(2, 0.02, 0.5, 0.8, 0.8)], 1, (2, 5)),
    'n65_F5_T128': (65, 5, 128, [(2, 0.2, 0.5, 0.5, 0.8), (1, 0.2, 1.0, 0.8, 0.3)], 3, ALL),
    'n65_F60_T1': (65, 60, 1, [(1, 0.2, 0.5, 0.8, 0.8), (2, 0.2, 1.0, 0.8, 0.8)], 1, (3, 5)),
    'n65_F128_T1': (65, 128, 1, [(2, 0.2, 1.0, 0.8, 0.8)], 3, (4, 5)),
    'n128_F1_T1': (128, 1, 1, [(2, 0.2, 0.5, 0.8, 0.8), (1, 0.2, 0.5, 0.5, 0.8)], 20, (0, 5)),
    'n128_F5_T128': (128, 5, 128, [(2, 0.2, 1.0, 0.8, 0.8)], 20, (2, 5)),
    'n128_F128_T128': (128, 128, 128, [(2, 0.2, 0.5, 0.8, 0.8), (1, 0.02, 1.0, 0.5, 0.8)], 1, (0, 5)),
}
assert {c[0] for c in CASES.values()} == {10, 63, 64, 65, 128} and {c[1] for c in CASES.values()} == {1, 5, 60, 128} and {c[2] for c in CASES.values()} == {1, 128}
assert {c[4] for c in CASES.values()} == {1, 3, 20} and {k[0] for c in CASES.values() for k in c[3]} == {1, 2}
CASE_SEED, FIT_SEED, N_SPLITS = 500, 7, 5
DUPLICATE, CONSTANT, THREE_VALUED = (0, 3), 1, 2      # from F = 5 on: column 3 repeats column 0, column 1 is constant, column 2 holds three values


def case_problem(label, p=0):
    """Problem p of a case: float32 x [n,F], y [n], test_x [T,F], test_y [T] and the stratified folds [n] int32 (dealt here, not by tabular: rows in class order
    get folds 0 .. 4 in turn, so every fold holds both classes where a class has five members).  From F = 5 on the planted columns above."""
    n, F, T = CASES[label][:3]
    x, y, tx, ty = tabular_cases.problem(n, F, T, CASE_SEED + 17 * sorted(CASES).index(label) + p)
    x, tx = x.copy(), tx.copy()
    if F >= 5:
        both = np.concatenate([x, tx])
        both[:, THREE_VALUED] = np.sign(np.round(both[:, THREE_VALUED]))
        both[:, DUPLICATE[1]] = both[:, DUPLICATE[0]]
        both[:, CONSTANT] = 0
        x, tx = both[:n], both[n:]
    folds = np.empty(n, dtype=np.int32)
    for k in (False, True):
        idx = np.flatnonzero((y > 0.5) == k)
        folds[idx] = np.arange(len(idx)) % N_SPLITS
    return x, y, tx, ty, folds


# the synthetic problems whose fits tests/golden/tabular_xgb.pt records for the structural comparison: (n, F, T, problem seed, rounds)
STRUCTURAL = [(24, 5, 6, 1, 20), (40, 8, 10, 2, 20), (80, 20, 20, 3, 3), (65, 8, 5, 4, 3)]
STRUCTURAL_CANDS = [(1, 0.2, 0.5, 0.8, 0.8), (2, 0.2, 0.5, 0.8, 0.8), (2, 0.02, 1.0, 0.5, 0.8)]
MIN_GAP, MIN_MCW_DISTANCE = 1e-4, 2. ** -16

# the windows of tests/golden/tabular_diabetes.pt behind the recorded full grid searches: (first row, train rows, test rows)
GRID_WINDOWS = [(0, 40, 20), (70, 40, 20)]

FAULTS = ('lambda_dropped', 'mcw_ignored', 'equal_values_split', 'unsampled_counted', 'k_off_by_one', 'tie_to_higher')


def diabetes_window(X, y, start, n, T):
    """Rows start .. start + n + T of the table as the study hands them to a baseline: normalised by the train rows' mean and std (ddof 1) + 1e-6, in f64, then f32."""
    raw = np.asarray(X, dtype=np.float64)[start:start + n + T]
    x = ((raw - raw[:n].mean(0)) / (raw[:n].std(0, ddof=1) + 1e-6)).astype(np.float32)
    yy = np.asarray(y, dtype=np.float32)[start:start + n + T]
    return x[:n], yy[:n], x[n:], yy[n:]
