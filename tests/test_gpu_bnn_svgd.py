"""SVGD on the BNN on the device (csrc/bnn_svgd.hip: pfn_bnn_svgd_steps) and what is built on it (mcmc_svi_transformer_on_bayesian.fit_bnn_svgd / BnnParticles /
eval_svgd) against the f64 restatement (tests/bnn_svgd_f64.py, verified on the host in tests/test_host_bnn_svgd.py against torch.median, torch.autograd and
torch.optim.Adam).

Bounds on continuous outputs: <= 2 x the value measured on the MI355X (profiles/r15_bnn_svgd_bounds_measured.json), and never above 1e-3.  Stein directions and
particles are compared relative to their norms, a bandwidth relative to itself, a one-step potential relative to |U|, the potentials of a trajectory relative
to max(1, |U|).  The invariants of the contract (a problem alone and in a batch, a run split over launches, untouched tails, a non-finite neighbour) are
compared bit for bit."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bnn_f64 as ref      # noqa: E402
import bnn_svgd_f64 as svgd      # noqa: E402
import bounds      # noqa: E402

from transformerscandobayesianinference_amd import hipops      # noqa: E402
from transformerscandobayesianinference_amd import mcmc_svi_transformer_on_bayesian as study      # noqa: E402

pytestmark = pytest.mark.gpu

DEV = 'cuda'
CAP = 1e-3
S = 100
BETA1 = float(np.float32(1) - np.float32(0.9))      # the kernel's 1 - beta1

# One step, P = 3: label -> (H, F, N, activation, n_of).  Every instantiation of the kernel: Hp 8 (H 1 / 5 / 8), Hp 16 (H 9 / 16), Hp 32 (H 17 / 32) and Hp 64
# (H 33 / 64), each with Fp 4 / 8 / 16 (F 1 / 3, 5 / 8, 16) and both activations; n of {0, 1, 63, 64, 65, 100} ragged over the problems; N of {2, 5, 50}, one more
# than four waves hold (33 at Hp 8, 17 at Hp 16, 9 at Hp 32, 5 at Hp 64) and one more than the block's eight waves hold (33 at Hp 16, 17 at Hp 32, 9 at Hp 64: the
# round loop, with a single particle in the second round; at Hp 8 the block holds all 64).  H 64 x F 16 x N 50 has D = 1218 (the state far beyond LDS: 20 tiles
# of columns, the last of 2; seven rounds), H 1 x F 1 has D = 6 (fewer coordinates than two waves take at a time).
ONE_STEP = {
    'H1_F1_i': (1, 1, 50, 'identity', (100, 0, 1)),
    'H5_F3_t': (5, 3, 50, 'tanh', (0, 63, 100)),
    'H8_F8_i': (8, 8, 33, 'identity', (1, 64, 65)),
    'H5_F5_t': (5, 5, 33, 'tanh', (65, 100, 0)),
    'H8_F16_i': (8, 16, 5, 'identity', (63, 64, 1)),
    'H1_F16_t': (1, 16, 2, 'tanh', (100, 65, 63)),
    'H9_F3_i': (9, 3, 17, 'identity', (64, 0, 100)),
    'H16_F1_t': (16, 1, 33, 'tanh', (1, 65, 63)),
    'H16_F8_i': (16, 8, 50, 'identity', (100, 63, 0)),
    'H9_F5_t': (9, 5, 5, 'tanh', (65, 1, 64)),
    'H16_F16_i': (16, 16, 2, 'identity', (0, 100, 65)),
    'H9_F16_t': (9, 16, 17, 'tanh', (63, 64, 100)),
    'H17_F3_i': (17, 3, 17, 'identity', (1, 100, 64)),
    'H32_F1_t': (32, 1, 9, 'tanh', (65, 0, 63)),
    'H17_F8_i': (17, 8, 9, 'identity', (100, 1, 65)),
    'H32_F5_t': (32, 5, 50, 'tanh', (64, 63, 0)),
    'H32_F16_i': (32, 16, 2, 'identity', (63, 65, 100)),
    'H17_F16_t': (17, 16, 9, 'tanh', (0, 64, 1)),
    'H33_F3_i': (33, 3, 9, 'identity', (100, 64, 0)),
    'H64_F1_t': (64, 1, 50, 'tanh', (63, 1, 65)),
    'H64_F8_i': (64, 8, 50, 'identity', (65, 100, 63)),
    'H33_F8_t': (33, 8, 5, 'tanh', (1, 0, 64)),
    'H33_F16_i': (33, 16, 2, 'identity', (64, 65, 1)),
    'H64_F16_t': (64, 16, 50, 'tanh', (100, 63, 0)),
}
# measured on the MI355X (profiles/r15_bnn_svgd_bounds_measured.json): (Stein direction, bandwidth, potential), each <= 2 x measured
ONE_STEP_BOUNDS = {
    'H1_F1_i': (3.1e-7, 2.8e-7, 2.9e-7),
    'H5_F3_t': (3.5e-7, 3.5e-7, 2.7e-7),
    'H8_F8_i': (3.2e-7, 3.3e-7, 3.2e-7),
    'H5_F5_t': (3.5e-7, 3.3e-7, 1.1e-7),
    'H8_F16_i': (3.5e-7, 3.1e-7, 9.4e-8),
    'H1_F16_t': (6.1e-7, 2.6e-7, 2.6e-7),
    'H9_F3_i': (3.4e-7, 3.4e-7, 3.6e-7),
    'H16_F1_t': (3.5e-7, 4.2e-7, 2.0e-8),
    'H16_F8_i': (3.5e-7, 4.1e-7, 4.8e-7),
    'H9_F5_t': (2.9e-7, 4.0e-7, 2.3e-7),
    'H16_F16_i': (3.3e-7, 3.8e-7, 4.1e-8),
    'H9_F16_t': (3.7e-7, 4.4e-7, 1.4e-7),
    'H17_F3_i': (4.0e-7, 3.7e-7, 5.3e-8),
    'H32_F1_t': (3.3e-7, 3.5e-7, 1.9e-7),
    'H17_F8_i': (2.9e-7, 3.7e-7, 1.1e-7),
    'H32_F5_t': (3.8e-7, 4.2e-7, 2.4e-7),
    'H32_F16_i': (3.2e-7, 4.3e-7, 1.5e-7),
    'H17_F16_t': (3.6e-7, 4.3e-7, 1.8e-7),
    'H33_F3_i': (3.2e-7, 4.1e-7, 2.9e-7),
    'H64_F1_t': (3.7e-7, 3.7e-7, 2.7e-7),
    'H64_F8_i': (4.1e-7, 4.4e-7, 1.6e-7),
    'H33_F8_t': (3.0e-7, 3.6e-7, 2.1e-7),
    'H33_F16_i': (3.0e-7, 3.9e-7, 9.9e-8),
    'H64_F16_t': (4.5e-7, 4.3e-7, 2.2e-7),
}
# Thirty steps: regime -> (H, F, N, n_of); by (regime, lr): (particles, potentials)
TRAJECTORY = {'resident': (5, 3, 9, (100, 63, 1)), 'tiled': (9, 8, 50, (65, 100, 0))}
TRAJECTORY_BOUNDS = {('resident', 0.001): (3.1e-7, 3.5e-7), ('resident', 0.05): (8.1e-7, 2.7e-7), ('tiled', 0.05): (1.5e-6, 5.6e-7)}
CHUNKED_BOUNDS = (1.4e-7, 4.2e-7)      # (particles, potentials)
HP_OF = lambda H: 8 if H <= 8 else 16 if H <= 16 else 32 if H <= 32 else 64      # launch_bnn_svgd_steps' dispatch
FP_OF = lambda F: 4 if F <= 4 else 8 if F <= 8 else 16
RESIDENT = lambda H, F, N: 16 * N * (ref.num_params(F, H) | 1) <= 66560      # bnn_svgd_resident: the state stays in LDS
assert {(HP_OF(c[0]), FP_OF(c[1]), c[3]) for c in ONE_STEP.values()} == {(hp, fp, act) for hp in (8, 16, 32, 64) for fp in (4, 8, 16) for act in ('identity', 'tanh')}
assert all(any(HP_OF(c[0]) == hp and c[2] == 256 // hp + 1 for c in ONE_STEP.values()) for hp in (8, 16, 32, 64))      # one more particle than four waves hold
assert all(any(HP_OF(c[0]) == hp and c[2] == 512 // hp + 1 for c in ONE_STEP.values()) for hp in (16, 32, 64))      # ... and than the block's eight hold
assert {2, 5, 50} <= {c[2] for c in ONE_STEP.values()} and {n for c in ONE_STEP.values() for n in c[4]} == {0, 1, 63, 64, 65, 100}
assert ONE_STEP['H64_F16_t'][:3] == (64, 16, 50) and ONE_STEP['H1_F1_i'][:2] == (1, 1)
assert {RESIDENT(*c[:3]) for c in ONE_STEP.values()} == {True, False} and RESIDENT(*TRAJECTORY['resident'][:3]) and not RESIDENT(*TRAJECTORY['tiled'][:3])
assert all(b <= CAP for v in list(ONE_STEP_BOUNDS.values()) + list(TRAJECTORY_BOUNDS.values()) + [CHUNKED_BOUNDS] for b in v)


def problem(H, F, N, P, seed, rows=S):
    """x [P,rows,F], y [P,rows] in {0, 1}, state [P, 3, N, D] with particles ~ N(0, 1) and zero moments, all f32 (the f64 side reads the same numbers)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(P, rows, F, generator=g)
    y = (torch.rand(P, rows, generator=g) > 0.5).float()
    return x, y, hipops.bnn_svgd_state(P, N, F, H, 'cpu', particles0=torch.randn(P, N, ref.num_params(F, H), generator=g))


def steps(x, y, state, H, num_steps, n_of=None, **kw):
    """hipops.bnn_svgd_steps on copies: (state after, potential, bandwidth), on the host."""
    n = None if n_of is None else torch.tensor(n_of, dtype=torch.int32, device=DEV)
    st = state.to(DEV).clone()
    pot, bw = hipops.bnn_svgd_steps(x.to(DEV), y.to(DEV), st, H, num_steps, n_of=n, **kw)
    return st.cpu(), pot.cpu(), bw.cpu()


def rel(got, want):
    """max over problems of |got - want| / |want| (norms over everything but the problem index)."""
    P = want.shape[0]
    return float(((got.double() - want).reshape(P, -1).norm(dim=1) / want.reshape(P, -1).norm(dim=1)).max())


@functools.lru_cache(maxsize=None)
def one_step_case(label):
    """Inputs and the f64 (mean U, h, s) of every problem of a case (computed once)."""
    H, F, N, activation, n_of = ONE_STEP[label]
    x, y, state = problem(H, F, N, 3, 3000 + sum(map(ord, label)))
    want = [svgd.step_terms(state[p, 0].double(), x[p], y[p], n_of[p], F, H, activation) for p in range(3)]
    return x, y, state, want


@pytest.mark.parametrize('label', list(ONE_STEP))
def test_one_step_against_f64(label):
    """From zero moments, m / (1 - beta1) after one step IS the Stein direction."""
    H, F, N, activation, n_of = ONE_STEP[label]
    D = ref.num_params(F, H)
    x, y, state, want = one_step_case(label)
    after, pot, bw = steps(x, y, state, H, 1, n_of=n_of, activation=activation)
    assert bool(torch.isfinite(after).all()) and bool(torch.isfinite(pot).all()) and bool(torch.isfinite(bw).all()) and bw.shape == (3, D)
    e_s = rel(after[:, 1] / BETA1, torch.stack([w[2] for w in want]))
    h64 = torch.stack([w[1] for w in want])
    e_h = float(((bw.double() - h64).abs() / h64).max())
    U64 = np.array([w[0] for w in want])
    e_U = float(np.max(np.abs(pot[:, 0].double().numpy() - U64) / np.abs(U64)))
    print(f'{label}: H {H} F {F} N {N} {activation} n_of {n_of}: direction {e_s:.3e}, bandwidth {e_h:.3e}, potential {e_U:.3e}')
    bounds.within(f'{label} direction', e_s, ONE_STEP_BOUNDS[label][0])
    bounds.within(f'{label} bandwidth', e_h, ONE_STEP_BOUNDS[label][1])
    bounds.within(f'{label} potential', e_U, ONE_STEP_BOUNDS[label][2])


def test_a_null_n_of_means_all_rows():
    x, y, state = problem(5, 3, 9, 3, 31)
    a1, p1, h1 = steps(x, y, state, 5, 4, n_of=(S, S, S), lr=0.05, activation='tanh')
    a2, p2, h2 = steps(x, y, state, 5, 4, lr=0.05, activation='tanh')
    assert torch.equal(a1, a2) and torch.equal(p1, p2) and torch.equal(h1, h2)
    assert not torch.equal(steps(x, y, state, 5, 4, n_of=(S, S - 1, S), lr=0.05, activation='tanh')[0][1], a2[1])


@functools.lru_cache(maxsize=None)
def trajectory_f64(regime, lr):
    H, F, N, n_of = TRAJECTORY[regime]
    x, y, state = problem(H, F, N, 3, 91)
    out = [svgd.run(state[p].double(), x[p], y[p], n_of[p], F, H, 'tanh', num_steps=30, lr=lr) for p in range(3)]
    return x, y, state, torch.stack([o[0] for o in out]), np.stack([o[1] for o in out]), torch.stack([o[2] for o in out])


@pytest.mark.parametrize('regime,lr', list(TRAJECTORY_BOUNDS))
def test_thirty_steps_against_f64(regime, lr):
    H, F, N, n_of = TRAJECTORY[regime]
    x, y, state, want_state, want_pot, want_h = trajectory_f64(regime, lr)
    after, pot, bw = steps(x, y, state, H, 30, n_of=n_of, lr=lr, activation='tanh')
    assert pot.shape == (3, 30) and bool(torch.isfinite(after).all()) and bool(torch.isfinite(pot).all())
    e_x = rel(after[:, 0], want_state[:, 0])
    e_U = float(np.max(np.abs(pot.double().numpy() - want_pot) / np.maximum(1., np.abs(want_pot))))
    print(f'30 steps, {regime}, lr {lr}: particles {e_x:.3e}, potentials {e_U:.3e}, last bandwidth {float(((bw.double() - want_h).abs() / want_h).max()):.3e}')
    bounds.within(f'{regime} lr {lr} particles', e_x, TRAJECTORY_BOUNDS[(regime, lr)][0])
    bounds.within(f'{regime} lr {lr} potentials', e_U, TRAJECTORY_BOUNDS[(regime, lr)][1])


def test_the_chunked_path_against_f64():
    """S = n = 1100 rows of 16 features: 75 KB, above the kernel's 48 KB budget for resident rows, so every round stages 64-row chunks; N = 33 at Hp 16 is two
    rounds, and D = 173 at N = 33 is the tiled regime."""
    H, F, N, T, rows = 9, 16, 33, 3, 1100
    assert not RESIDENT(H, F, N) and rows * (FP_OF(F) + 1) * 4 > 48 * 1024
    x, y, state = problem(H, F, N, 1, 17, rows=rows)
    want_state, want_pot, _ = svgd.run(state[0].double(), x[0], y[0], rows, F, H, 'tanh', num_steps=T, lr=0.01)
    after, pot, _ = steps(x, y, state, H, T, lr=0.01, activation='tanh')
    e_x = rel(after[:, 0], want_state[None, 0])
    e_U = float(np.max(np.abs(pot.double().numpy() - want_pot[None]) / np.maximum(1., np.abs(want_pot[None]))))
    print(f'chunked: particles {e_x:.3e}, potentials {e_U:.3e}')
    bounds.within('chunked particles', e_x, CHUNKED_BOUNDS[0])
    bounds.within('chunked potentials', e_U, CHUNKED_BOUNDS[1])


# (H, F, N, activation): resident in one round, tiled (D = 101: one full tile and one of 37 columns; two rounds), tiled at Hp 64 and resident at Hp 64 (two rounds each)
BITWISE = [(5, 3, 50, 'tanh'), (9, 8, 50, 'identity'), (64, 16, 9, 'tanh'), (33, 1, 9, 'identity')]
assert [RESIDENT(*c[:3]) for c in BITWISE] == [True, False, False, True]


@pytest.mark.parametrize('H,F,N,activation', BITWISE)
def test_a_problem_is_a_bitwise_function_of_its_own_inputs(H, F, N, activation):
    """(a) Problem q of a P = 3 call against the same problem alone, and the batch reversed."""
    n_of = (65, 7, 100)
    x, y, state = problem(H, F, N, 3, 400 + H)
    after, pot, bw = steps(x, y, state, H, 5, n_of=n_of, lr=0.05, activation=activation)
    assert bool(torch.isfinite(after).all())
    for q in range(3):
        a1, p1, h1 = steps(x[q:q + 1], y[q:q + 1], state[q:q + 1], H, 5, n_of=n_of[q:q + 1], lr=0.05, activation=activation)
        assert torch.equal(a1[0], after[q]) and torch.equal(p1[0], pot[q]) and torch.equal(h1[0], bw[q]), q
    a2, p2, h2 = steps(x.flip(0).contiguous(), y.flip(0).contiguous(), state.flip(0).contiguous(), H, 5, n_of=n_of[::-1], lr=0.05, activation=activation)
    assert torch.equal(a2.flip(0), after) and torch.equal(p2.flip(0), pot) and torch.equal(h2.flip(0), bw)


@pytest.mark.parametrize('H,F,N', [(5, 3, 50), (9, 8, 50)])
def test_a_run_split_over_launches_is_the_same_run(H, F, N):
    """(b) steps(0, 20) against steps(0, 7) then steps(7, 13), in both regimes."""
    x, y, state = problem(H, F, N, 3, 21)
    kw = dict(n_of=(100, 64, 3), lr=0.05, activation='tanh')
    whole, pot, bw = steps(x, y, state, H, 20, **kw)
    first, p1, _ = steps(x, y, state, H, 7, **kw)
    second, p2, h2 = steps(x, y, first, H, 13, step0=7, **kw)
    assert torch.equal(second, whole) and torch.equal(torch.cat([p1, p2], 1), pot) and torch.equal(h2, bw)
    assert not torch.equal(steps(x, y, first, H, 13, step0=0, **kw)[0], whole)      # step0 counts: the bias corrections follow it


def test_fit_bnn_svgd_does_not_depend_on_the_launch_length():
    H, F = 5, 3
    x, y, _ = problem(H, F, 2, 3, 22)
    spec = dict(num_features=F, embed=H)
    fits = [study.fit_bnn_svgd(x.to(DEV), y.to(DEV), spec, n_of=[100, 64, 3], num_steps=20, lr=0.05, num_particles=50, seed=2, activation='tanh', steps_per_launch=per)
            for per in (1, 7, 256)]
    assert fits[0].potentials.shape == (3, 20) and fits[0].particles.shape == (3, 50, 32) and bool(torch.isfinite(fits[0].state).all())
    for f in fits[1:]:
        assert torch.equal(f.state, fits[0].state) and torch.equal(f.potentials, fits[0].potentials)
    # the start is the median of 15 draws per coordinate, drawn on the host
    zero = study.fit_bnn_svgd(x.to(DEV), y.to(DEV), spec, num_steps=0, num_particles=50, seed=2)
    assert torch.equal(zero.particles.cpu(), svgd.initial_particles(3, 50, 32, 2)) and zero.potentials.shape == (3, 0)


@pytest.mark.parametrize('H,F,N', [(5, 3, 9), (9, 8, 50)])
def test_rows_beyond_n_columns_beyond_d_and_the_bytes_after_every_output_are_never_touched(H, F, N):
    """(c) NaN in the rows >= n of x / y, a sentinel in the columns >= D of a state and a bandwidth with ld = D + 5, a canary band behind each output."""
    n_of = (0, 63, 99)
    D, T, band = ref.num_params(F, H), 6, 64
    x, y, state = problem(H, F, N, 3, 77)
    clean, clean_pot, clean_bw = steps(x, y, state, H, T, n_of=n_of, lr=0.05, activation='tanh')
    xp, yp = x.clone(), y.clone()
    for p, n in enumerate(n_of):
        xp[p, n:], yp[p, n:] = float('nan'), float('nan')
    ld = D + 5
    st_buf = torch.full((3 * 3 * N * ld + band,), -777., device=DEV)
    pot_buf = torch.full((3 * T + band,), -777., device=DEV)
    bw_buf = torch.full((3 * ld + band,), -777., device=DEV)
    wide, pot, bw = st_buf[:3 * 3 * N * ld].view(3, 3, N, ld), pot_buf[:3 * T].view(3, T), bw_buf[:3 * ld].view(3, ld)
    wide[..., :D] = state.to(DEV)
    hipops.bnn_svgd_steps(xp.to(DEV), yp.to(DEV), wide, H, T, n_of=torch.tensor(n_of, dtype=torch.int32, device=DEV), lr=0.05, activation='tanh', potential=pot, bandwidth=bw)
    assert bool((wide[..., D:] == -777.).all()) and bool((bw[:, D:] == -777.).all())
    assert bool((st_buf[-band:] == -777.).all()) and bool((pot_buf[-band:] == -777.).all()) and bool((bw_buf[-band:] == -777.).all())
    assert torch.equal(wide[..., :D].cpu(), clean) and torch.equal(pot.cpu(), clean_pot) and torch.equal(bw[:, :D].cpu(), clean_bw)
    assert bool(torch.isfinite(clean).all()) and bool(torch.isfinite(clean_pot).all()) and bool(torch.isfinite(clean_bw).all())


@pytest.mark.parametrize('H,F,N', [(9, 5, 17), (9, 8, 50)])
def test_a_non_finite_problem_stays_alone(H, F, N):
    """(d) One particle of one problem is NaN: that problem goes non-finite, the others are the bits of a run without it."""
    x, y, state = problem(H, F, N, 3, 5)
    good, good_pot, good_bw = steps(x, y, state, H, 6, lr=0.05)
    bad = state.clone()
    bad[1, 0, 2, 3] = float('nan')
    after, pot, bw = steps(x, y, bad, H, 6, lr=0.05)
    assert not bool(torch.isfinite(after[1, 0]).all()) and not bool(torch.isfinite(pot[1]).any())
    assert torch.equal(after[[0, 2]], good[[0, 2]]) and torch.equal(pot[[0, 2]], good_pot[[0, 2]]) and torch.equal(bw[[0, 2]], good_bw[[0, 2]])


def test_with_no_data_the_particles_spread_over_the_prior():
    """n_of = 0: the target is N(0, I).  tests/test_host_bnn_svgd.py shows the restatement alone meets the same three conditions from the same start (max |mean|
    1.2e-3, max |std - 1| 0.025, the potential rising from 31.0 to 44.4 there)."""
    c = svgd.NO_DATA
    state = hipops.bnn_svgd_state(c['P'], c['N'], c['F'], c['H'], 'cpu', particles0=svgd.no_data_start())
    x, y = torch.zeros(c['P'], 1, c['F']), torch.zeros(c['P'], 1)
    after, pot, _ = steps(x, y, state, c['H'], c['T'], n_of=[0] * c['P'], lr=c['lr'])
    mean, std, rise = svgd.no_data_conditions(after[:, 0], pot.numpy())
    print(f'no data: max |mean| {mean:.2e}, max |std - 1| {std:.3f}, potential {float(pot[:, 0].mean()):.2f} -> {float(pot[:, -50:].mean()):.2f} (min rise {rise:.2f})')
    bounds.within('no data max |mean|', mean, 0.05)      # the issue's conditions, with their values on record
    bounds.within('no data max |std - 1|', std, 0.1)
    assert rise > 0.


def test_eval_svgd_on_toy_data():
    spec = study.get_default_model_spec('small')
    model = study.BayesianModel(spec, device=DEV)
    X, y = study.generate_toy_data(model, 30, device=DEV)
    X, y = X[:4], y[:4]
    nll, acc = study.eval_svgd(X, y, DEV, spec, 10, num_train_steps=40)
    assert isinstance(nll, np.ndarray) and isinstance(acc, np.ndarray) and nll.shape == (4,) and acc.shape == (4,)
    assert np.isfinite(nll).all() and np.isfinite(acc).all() and (acc >= 0).all() and (acc <= 1).all() and (nll > 0).all()
    nll2, acc2 = study.eval_svgd(X, y, DEV, spec, 10, num_train_steps=40, num_pred_samples=7)      # num_pred_samples: accepted and ignored
    assert np.array_equal(nll, nll2) and np.array_equal(acc, acc2)
    nll3, acc3 = study.eval_svgd(X, y, DEV, lambda: study.BayesianModel(spec, device=DEV), 10, num_train_steps=40)      # a model sampler in place of the spec
    assert np.array_equal(nll, nll3) and np.array_equal(acc, acc3)
    nll4, acc4 = study.eval_svgd(X, y, DEV, spec, 10, num_train_steps=40, sample_obs=True)      # the reference's estimator
    assert nll4.shape == (4,) and acc4.shape == (4,) and np.isfinite(nll4).all() and (acc4 >= 0).all() and (acc4 <= 1).all()
    # the predictive is the particles: prob1 [P, N, m] of pfn_bnn_predict against the f64 predictive
    fit = study.fit_bnn_svgd(X[:, :10].contiguous(), y[:, :10].contiguous(), spec, num_steps=40, num_particles=50, seed=0)
    prob = fit.predictive(X[:, 10:].contiguous())
    assert fit.particles.shape == (4, 50, 32) and prob.shape == (4, 50, 20) and bool(((prob >= 0) & (prob <= 1)).all())
    for p, i in ((0, 0), (3, 49)):
        assert float((ref.predict(fit.particles[p, i].double().cpu(), X[p, 10:].cpu(), 3, 5) - prob[p, i].double().cpu()).abs().max()) < 1e-5
    # the 'big' spec (D = 706: the tiled regime) runs
    big = study.get_default_model_spec('big')
    Xb = torch.randn(3, 20, 8, generator=torch.Generator().manual_seed(1)).to(DEV)
    yb = (torch.rand(3, 20, generator=torch.Generator().manual_seed(2)) > 0.5).float().to(DEV)
    nll5, acc5 = study.eval_svgd(Xb, yb, DEV, big, 12, num_train_steps=30)
    assert nll5.shape == (3,) and np.isfinite(nll5).all() and np.isfinite(acc5).all() and (nll5 > 0).all()


def test_training_steps_writes_the_references_files(tmp_path):
    """training_steps('svgd', ...), the call of the reference's __main__: 2 .. 4096 steps, one file each."""
    spec = study.get_default_model_spec('small')
    g = torch.Generator().manual_seed(3)
    X, y = torch.randn(3, 104, 3, generator=g), (torch.rand(3, 104, generator=g) > 0.5).float()
    study.training_steps('svgd', X, y, spec, device=DEV, path_interfix=str(tmp_path))
    assert sorted(f.name for f in tmp_path.iterdir()) == sorted(f'results_svgd_training_steps_{s}.npy' for s in (2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096))
    for s in (2, 4096):
        nll, acc, seconds = np.load(tmp_path / f'results_svgd_training_steps_{s}.npy', allow_pickle=True)
        assert nll.shape == (3,) and acc.shape == (3,) and np.isfinite(nll).all() and (acc >= 0).all() and (acc <= 1).all() and seconds > 0
