"""f64 restatement of the NUTS state machine of csrc/gp_mcmc.hip, in numpy on the CPU: the same Philox4x32-10 draws, `u01` and
Box-Muller from the same 32-bit words, the iterative multinomial transition with its checkpoint rows, a recursive build-tree variant of the same
transition (the textbook formulation, to verify the iterative one), and the dual-averaging / mass-window recurrences of the warmup.

Every transition also reports its DECISION MARGIN: the minimum over all decisions it took of |u - p| for a uniform compared with a probability p < 1
(|u - 1/2| for the direction), |dot| / (|m a| |s'|) for a U-turn product and |dE - 1000| / 1000 for the divergence test.  An f32 run of the same
transition can take another branch only where that margin is of the order of f32 round-off, so tests leave chains with a tiny margin out of an exact
comparison of the discrete outcomes."""
import math

import numpy as np

M32 = 0xFFFFFFFF


def philox4x32_10(idx, stream, seed):
    c0, c1, c2, c3 = idx & M32, (idx >> 32) & M32, stream & M32, (stream >> 32) & M32
    k0, k1 = seed & M32, (seed >> 32) & M32
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & M32, p1 & M32, ((p0 >> 32) ^ c3 ^ k1) & M32, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def u01(r):
    return (r >> 8) * 2. ** -24


def u01_open(r):
    return ((r >> 8) + 1.) * 2. ** -24


def normal4(block):
    x, y, z, w = block
    r0, r1 = math.sqrt(-2. * math.log(u01_open(x))), math.sqrt(-2. * math.log(u01_open(z)))
    a0, a1 = 2. * math.pi * u01(y), 2. * math.pi * u01(w)
    return r0 * math.cos(a0), r0 * math.sin(a0), r1 * math.cos(a1), r1 * math.sin(a1)


class Draws:
    """The random numbers of one chain: idx = (transition << 12) | slot; slots 0-31 the momentum normals (coordinate k: block k >> 2, component k & 3),
    slot 32 + j: (u_dir[j], u_top[j]) in (.x, .y), slot 64 + (l >> 2) component l & 3: u_leaf[l]."""

    def __init__(self, seed, chain_id):
        self.seed, self.chain_id = int(seed), int(chain_id)

    def block(self, t, slot):
        return philox4x32_10((int(t) << 12) | slot, self.chain_id, self.seed)

    def momentum(self, t, D):
        z = []
        for b in range((D + 3) // 4):
            z.extend(normal4(self.block(t, b)))
        return np.array(z[:D])

    def dir_top(self, t, j):
        b = self.block(t, 32 + j)
        return u01(b[0]), u01(b[1])

    def leaf(self, t, l):
        return u01(self.block(t, 64 + (l >> 2))[l & 3])


def logaddexp(a, b):
    hi, lo = max(a, b), min(a, b)
    return hi if hi == -math.inf else hi + math.log1p(math.exp(lo - hi))


class Margin:
    def __init__(self):
        self.value = math.inf

    def uniform(self, u, p):
        if p < 1.:
            self.value = min(self.value, abs(u - p))

    def turn(self, m, a, b, s):
        sp = s - 0.5 * (a + b)
        out = False
        for v in (a, b):
            d = float(np.sum(m * v * sp))
            den = float(np.linalg.norm(m * v) * np.linalg.norm(sp))
            self.value = min(self.value, abs(d) / den if den > 0 else 0.)
            out = out or d <= 0.
        return out

    def energy(self, dE):
        self.value = min(self.value, abs(dE - 1000.) / 1000.)


def _evaluate(fun, theta):
    U, g = fun(theta)
    U = float(U)
    if not math.isfinite(U):
        return math.inf, np.zeros_like(theta)
    return U, np.asarray(g, dtype=np.float64)


def transition(fun, theta, U, g, m, eps, draws, t, max_tree_depth):
    """One iterative multinomial NUTS transition from (theta, U, g = grad U) with inverse mass m and step eps.  fun(theta) -> (U, grad).
    Returns dict(theta, U, g, depth, leapfrogs, diverging, accept, margin)."""
    D = len(theta)
    mg = Margin()
    r0 = draws.momentum(t, D) / np.sqrt(m)
    H0 = U + 0.5 * float(np.sum(m * r0 * r0))
    left, right = [theta.copy(), r0.copy(), g.copy()], [theta.copy(), r0.copy(), g.copy()]
    prop, logW, rsum, depth, leaves, accept_sum, diverging = (theta.copy(), U, g.copy()), 0., r0.copy(), 0, 0, 0., 0
    while True:
        u_dir, u_top = draws.dir_top(t, depth)
        mg.uniform(u_dir, 0.5)
        v = 1. if u_dir < 0.5 else -1.
        edge = right if v > 0 else left
        n, s_logW, s_rsum, s_prop, ended = 0, -math.inf, np.zeros(D), None, False
        r_ck, s_ck = {}, {}
        while n < 2 ** depth:
            th, r, gg = edge
            r = r - 0.5 * v * eps * gg
            th = th + v * eps * m * r
            Un, gn = _evaluate(fun, th)
            r = r - 0.5 * v * eps * gn
            edge[0], edge[1], edge[2] = th, r, gn
            dE = Un + 0.5 * float(np.sum(m * r * r)) - H0
            fin = math.isfinite(dE)
            accept_sum += min(1., math.exp(min(-dE, 0.))) if fin else 0.
            leaves += 1
            if fin:
                mg.energy(dE)
            if not fin or dE > 1000.:
                diverging, ended = 1, True
                break
            new = logaddexp(s_logW, -dE)
            p = math.exp(min(-dE - new, 0.))
            u = draws.leaf(t, leaves - 1)
            mg.uniform(u, p)
            if u < p:
                s_prop = (th.copy(), Un, gn.copy())
            s_logW = new
            s_rsum = s_rsum + r
            if n % 2 == 0:
                i = bin(n >> 1).count('1')
                r_ck[i], s_ck[i] = r.copy(), s_rsum.copy()
            else:
                imax = bin(n >> 1).count('1')
                ones = 0
                while (n >> ones) & 1:
                    ones += 1
                for i in range(imax, imax - ones, -1):
                    if mg.turn(m, r_ck[i], r, s_rsum - s_ck[i] + r_ck[i]):
                        ended = True
                        break
                if ended:
                    n += 1
                    break
            n += 1
        if ended:
            depth_out = depth + 1
            break
        p = min(1., math.exp(min(s_logW - logW, 0.)))
        mg.uniform(u_top, p)
        if u_top < p:
            prop = s_prop
        logW = logaddexp(logW, s_logW)
        rsum = rsum + s_rsum
        depth += 1
        depth_out = depth
        if mg.turn(m, left[1], right[1], rsum) or depth >= max_tree_depth:
            break
    return dict(theta=prop[0], U=prop[1], g=prop[2], depth=depth_out, leapfrogs=leaves, diverging=diverging, accept=accept_sum / leaves, margin=mg.value)


def transition_recursive(fun, theta, U, g, m, eps, draws, t, max_tree_depth):
    """The same trajectory by recursive doubling (Hoffman & Gelman's BuildTree with the generalised U-turn criterion on the summed momenta): only the
    discrete outcome -- (depth, leapfrogs, diverging) -- which depends on the dynamics and the directions, not on which point is kept."""
    D = len(theta)
    r0 = draws.momentum(t, D) / np.sqrt(m)
    H0 = U + 0.5 * float(np.sum(m * r0 * r0))
    count = [0]

    def turn(a, b, s):
        sp = s - 0.5 * (a + b)
        return float(np.sum(m * a * sp)) <= 0. or float(np.sum(m * b * sp)) <= 0.

    def build(state, v, j):
        """-> (first momentum, last momentum, sum of momenta, last state, stop, diverged) of 2^j leaves continuing from state in direction v."""
        if j == 0:
            th, r, gg = state
            r = r - 0.5 * v * eps * gg
            th = th + v * eps * m * r
            Un, gn = _evaluate(fun, th)
            r = r - 0.5 * v * eps * gn
            count[0] += 1
            dE = Un + 0.5 * float(np.sum(m * r * r)) - H0
            bad = not math.isfinite(dE) or dE > 1000.
            return r, r, r.copy(), (th, r, gn), bad, bad
        a1, b1, s1, state, stop, div = build(state, v, j - 1)
        if stop:
            return a1, b1, s1, state, True, div
        a2, b2, s2, state, stop, div = build(state, v, j - 1)
        s = s1 + s2
        return a1, b2, s, state, stop or turn(a1, b2, s), div

    left, right, rsum, depth = (theta, r0, g), (theta, r0, g), r0.copy(), 0
    diverging = 0
    while True:
        v = 1. if draws.dir_top(t, depth)[0] < 0.5 else -1.
        _, _, s, state, stop, div = build(right if v > 0 else left, v, depth)
        if stop:
            diverging = int(div)
            depth += 1
            break
        if v > 0:
            right = state
        else:
            left = state
        rsum = rsum + s
        depth += 1
        if turn(left[1], right[1], rsum) or depth >= max_tree_depth:
            break
    return dict(depth=depth, leapfrogs=count[0], diverging=diverging)


class Adaptation:
    """The warmup recurrences: dual averaging of the step size (gamma .05, t0 10, kappa .75, mu = log(10 eps)) and the Welford mean / M2 of the kept
    points over the slow windows [(start, end), ...]; at a window's end m = var n / (n + 5) + 1e-3 * 5 / (n + 5) and dual averaging restarts."""

    def __init__(self, step_size, target, W, windows, inv_mass):
        self.eps, self.target, self.W = float(step_size), float(target), int(W)
        self.ends = [e for _, e in windows]
        self.start = windows[0][0] if windows else 0
        self.m = np.array(inv_mass, dtype=np.float64)
        self.mu, self.count, self.hbar, self.leb = math.log(10. * self.eps), 0, 0., 0.
        self.window, self.wn, self.mean, self.m2 = 0, 0, np.zeros_like(self.m), np.zeros_like(self.m)

    def update(self, t, accept, kept):
        """After warmup transition t (< W) that kept `kept` with mean accept probability `accept`."""
        self.count += 1
        w = 1. / (self.count + 10.)
        self.hbar = (1. - w) * self.hbar + w * (self.target - accept)
        le = self.mu - math.sqrt(self.count) / 0.05 * self.hbar
        eta = self.count ** -0.75
        self.leb = eta * le + (1. - eta) * self.leb
        self.eps = math.exp(le)
        if self.window < len(self.ends) and t >= self.start:
            self.wn += 1
            d = kept - self.mean
            self.mean = self.mean + d / self.wn
            self.m2 = self.m2 + d * (kept - self.mean)
            if t + 1 == self.ends[self.window]:
                if self.wn > 1:
                    n = float(self.wn)
                    self.m = self.m2 / (n - 1.) * (n / (n + 5.)) + 1e-3 * (5. / (n + 5.))
                self.mean, self.m2, self.wn = np.zeros_like(self.m), np.zeros_like(self.m), 0
                self.window += 1
                self.mu, self.count, self.hbar, self.leb = math.log(10. * self.eps), 0, 0., 0.
        if t + 1 == self.W:
            self.eps = math.exp(self.leb)


def run_chain(fun, theta0, num_samples, warmup, seed, chain_id, step_size=0.1, target_accept=0.8, max_tree_depth=10, windows=(), inv_mass=None):
    """A whole chain in f64.  Returns dict(samples [N,D], warm [W,D], stats [W+N,8], inv_mass, margin [W+N])."""
    theta = np.array(theta0, dtype=np.float64)
    D = len(theta)
    draws = Draws(seed, chain_id)
    ad = Adaptation(step_size, target_accept, warmup, list(windows), np.ones(D) if inv_mass is None else inv_mass)
    U, g = _evaluate(fun, theta)
    points, stats, margins = [], [], []
    for t in range(warmup + num_samples):
        eps = ad.eps
        res = transition(fun, theta, U, g, ad.m, eps, draws, t, max_tree_depth)
        theta, U, g = res['theta'], res['U'], res['g']
        points.append(theta.copy())
        stats.append([eps, res['accept'], res['depth'], res['leapfrogs'], res['diverging'], U, 0., 0.])
        margins.append(res['margin'])
        if t < warmup:
            ad.update(t, res['accept'], theta)
    points = np.array(points).reshape(warmup + num_samples, D)
    return dict(samples=points[warmup:], warm=points[:warmup], stats=np.array(stats), inv_mass=ad.m, margin=np.array(margins))


# ---------------------------------------------------------------------------------------------------------------------
# The GP hyper-posterior the sampler is checked on: F = 1, n = 12, Matern 5/2, outputscale_concentration = 2
# ---------------------------------------------------------------------------------------------------------------------
GP_HP = {'outputscale_concentration': 2.}
GP_BOX = ((-4.5, 3., 70), (-5., 6., 70), (-14., 3., 110))      # log lengthscale, log outputscale, eta = log(noise - floor): (lo, hi, points)


def gp_problem():
    """(x [12,1], y [12] f32, prior [8] f64, kernel) of the test problem."""
    import torch
    import gp_fit_f64 as ref
    from transformerscandobayesianinference_amd.priors import fast_gp_mix
    prior = fast_gp_mix.hyperprior_vector(GP_HP, dtype=torch.float64)
    x, y = ref.make_problems(1, 12, 1, 1, seed=4, prior=prior)
    return x[0], y[0], prior, 1


def gp_potential_autograd(x, y, prior, kernel, n=None):
    """fun(theta [F+2]) -> (U, grad U) in f64 for U = n J(theta, mean 0) - sum theta (the target of priors.fast_gp_mix.sample_hyperparameter_posterior),
    from gp_fit_f64's objective by autograd."""
    import torch
    import gp_fit_f64 as ref
    n = x.shape[0] if n is None else int(n)

    def fun(theta):
        t = torch.cat([torch.as_tensor(theta, dtype=torch.float64), torch.zeros(1, dtype=torch.float64)])
        try:
            J, g = ref.value_and_grad(t, x, y, n, prior, kernel, fit_mean=False)
        except Exception:      # a failed factorisation: a divergent leaf
            return math.inf, np.zeros(len(theta))
        return n * float(J) - float(t.sum()), n * g[:-1].numpy() - 1.
    return fun


def gp_potential(x, y, prior, kernel, n=None):
    """The same function for Matern 5/2 in closed form in numpy (an autograd call costs 20 x as much; the host test checks the two against each other)."""
    assert kernel == 1
    n = x.shape[0] if n is None else int(n)
    X, Y, pr = np.asarray(x, dtype=np.float64)[:n], np.asarray(y, dtype=np.float64)[:n], np.asarray(prior, dtype=np.float64)
    F = X.shape[1]
    d2 = (X[:, None, :] - X[None, :, :]) ** 2      # [n, n, F]
    const = 0.5 * n * math.log(2 * math.pi) - sum(a * math.log(b) - math.lgamma(a) for a, b in ((pr[0], pr[1]),) * F + ((pr[2], pr[3]), (pr[4], pr[5])))

    def fun(theta):
        theta = np.asarray(theta, dtype=np.float64)
        ls, os_, en = np.exp(theta[:F]), math.exp(theta[F]), math.exp(theta[F + 1])
        noise = en + pr[6]
        q = d2 / (ls * ls)
        sq = np.sqrt(5. * q.sum(-1))
        e = np.exp(-sq)
        k = (1. + sq + sq * sq / 3.) * e
        try:
            L = np.linalg.cholesky(os_ * k + noise * np.eye(n))
        except np.linalg.LinAlgError:
            return math.inf, np.zeros(F + 2)
        Kinv = np.linalg.inv(L)
        Kinv = Kinv.T @ Kinv
        al = Kinv @ Y
        A = 0.5 * (Kinv - np.outer(al, al))
        U = 0.5 * float(Y @ al) + float(np.log(np.diag(L)).sum()) + const
        U -= float(((pr[0] - 1.) * theta[:F] - pr[1] * ls).sum()) + (pr[2] - 1.) * theta[F] - pr[3] * os_ + (pr[4] - 1.) * math.log(noise) - pr[5] * noise
        U -= float(theta.sum())
        g = np.empty(F + 2)
        dk = (5. / 3.) * (1. + sq) * e
        for d in range(F):
            g[d] = float((A * (os_ * dk * q[:, :, d])).sum()) - ((pr[0] - 1.) - pr[1] * ls[d]) - 1.
        g[F] = float((A * (os_ * k)).sum()) - ((pr[2] - 1.) - pr[3] * os_) - 1.
        g[F + 1] = float(np.trace(A)) * en - ((pr[4] - 1.) / noise - pr[5]) * en - 1.
        return U, g
    return fun


_quadrature = {}


def gp_quadrature():
    """Posterior means of (log l, log os, eta) of the test problem by f64 grid quadrature on GP_BOX, and the share of the mass that sits on the box faces."""
    if _quadrature:
        return _quadrature['mean'], _quadrature['face_mass']
    import torch
    import gp_fit_f64 as ref
    x, y, prior, kernel = gp_problem()
    x, y, n = x.double(), y.double(), x.shape[0]
    axes = [torch.linspace(lo, hi, k, dtype=torch.float64) for lo, hi, k in GP_BOX]
    logp = torch.empty(len(axes[0]), len(axes[1]), len(axes[2]), dtype=torch.float64)
    eye = torch.eye(n, dtype=torch.float64)
    lg = lambda v, a, b: (a - 1) * torch.log(v) - b * v
    for i, ll in enumerate(axes[0]):
        k0 = ref.cov(x, x, ll.exp().reshape(1), kernel)
        os_, noise = axes[1].exp()[:, None], axes[2].exp()[None, :] + prior[6]
        K = os_[:, :, None, None] * k0 + noise[:, :, None, None] * eye      # [70, 110, n, n]
        L = torch.linalg.cholesky(K)
        w = torch.linalg.solve_triangular(L, y.reshape(1, 1, n, 1).expand(K.shape[0], K.shape[1], n, 1), upper=False)[..., 0]
        ll_data = -0.5 * (w * w).sum(-1) - torch.log(torch.diagonal(L, dim1=-2, dim2=-1)).sum(-1)
        logp[i] = ll_data + lg(ll.exp(), prior[0], prior[1]) + lg(os_, prior[2], prior[3]) + lg(noise, prior[4], prior[5]) + ll + axes[1][:, None] + axes[2][None, :]
    wgt = (logp - logp.max()).exp()
    total = wgt.sum()
    mean = np.array([float((wgt.sum((1, 2)) * axes[0]).sum() / total), float((wgt.sum((0, 2)) * axes[1]).sum() / total), float((wgt.sum((0, 1)) * axes[2]).sum() / total)])
    face = wgt[0].sum() + wgt[-1].sum() + wgt[:, 0].sum() + wgt[:, -1].sum() + wgt[:, :, 0].sum() + wgt[:, :, -1].sum()
    _quadrature['mean'], _quadrature['face_mass'] = mean, float(face / total)
    return _quadrature['mean'], _quadrature['face_mass']
