"""Longdouble references, comparators, mutants and a NumPy stand-in for joint posterior sampling, Thompson picks and Monte-Carlo
q-EI (NumPy / SciPy only; data and references of tests/test_sample_host.py, tests/test_gpu_sample.py and tests/test_gpu_qei.py, not
product code).  Conventions of tests/chol_stability_ref.py and tests/posterior_ref.py: u = 2^-53, residuals in np.longdouble.

What is judged, and why in this form.  The Cholesky factor of a nearly singular covariance is NOT stable in the forward sense (two
correct factorisations of C + nugget I differ by cond * u), only F F^T is.  So nothing here compares a factor, or samples drawn from
it, against a factor computed elsewhere:

  factor     |F F^T - Chat|_ij <= c (M + 1) u sqrt(Chat_ii Chat_jj),  Chat = C_dev + nugget I formed in float64 as the device forms
             it (one addition per diagonal entry, bit for bit), c = chol_stability_ref.MARGIN = 8: the constant the device's
             factorisation is already held to there; no new one.  (M + 1) u is Higham's Thm 10.3 bound gamma_{M+1}, to first
             order, on |K - L L^T| / (|L||L^T|) for ANY ordering of the inner products, and |L||L^T|_ij <= sqrt((L L^T)_ii (L L^T)_jj)
             by Cauchy-Schwarz.  LAPACK sits near 0.06 (M + 1) u on these matrices; a leaf that multiplies by explicit inverses of
             its diagonal blocks (chol_stability_ref.chol_block_inverse, order 128) reaches 18 (M + 1) u on the most rank-deficient
             of them (squared exponential, N = 40, M = 129), which is why the sampler refines its factor by one step.
  draw       |out - (mean + F xi)|_sj <= (M + 2) u (|mean_j| + (|F| |xi_s|)_j), the replay in longdouble from the device's OWN F and
             mean: a sum of at most M products and the mean, in any order, then stored (gamma_{M+1} to first order, one unit spare).
  arg-best   exact: the first arg-min / arg-max of the device's own rows.
  q-EI       |cost - replay| <= max_s e_s + (ceil(log2 S) + 1) u |cost|,  e_s = (q + 2) u max_j (|mu_j| + (|F| |xi_s|)_j), the replay
             in longdouble from the device's own mean_b, F_b and xi.  Derivation: min and max(0, .) are 1-Lipschitz, so a sample's
             value v_s = max(0, fBest - min_j f_sj) moves by at most the worst error of its f_sj, which is the draw bound with q for
             M; the average of S such errors is at most their maximum.  The sum of the S non-negative values through a tree of depth
             ceil(log2 S) carries gamma_depth relative, the division by S one more rounding: (ceil(log2 S) + 1) u |cost|.  One
             rounding of the device is not named by that count: fBest - min, relative u on every term, u |cost| on the average.
             When S is a power of two the division is exact and the count holds as it stands.  Otherwise the draw bound's spare
             unit takes it (a chain of j + 1 fused multiply-adds and one addition makes q + 1 of the q + 2 roundings charged),
             which covers it while |cost| <= max_s max_j (|mu_j| + (|F| |xi_s|)_j); beyond that (fBest far above every mean) the
             kernel's first-order worst case is one u |cost| above the bound, which stays as the issue states it.  Nothing is
             measured.
"""
import math

import numpy as np
import scipy.linalg as sl
import scipy.special as ssp

import chol_stability_ref as CR
import design_replay_ref as DR
import kernel_reference as KR
import posterior_ref as P

LD, U = CR.LD, CR.U
QEI_MAX_Q = 32


# ---- cases -------------------------------------------------------------------------------------------------------------------------
def kernel_spec(kind, d):
    if kind == "se":
        return dict(kind="se", d=d, cl=[0.5 + 0.05 * k for k in range(d)], signalSize=1.2)
    if kind in ("matern32", "matern52"):
        return dict(kind=kind, d=d, rho=0.7, signalSize=1.1)
    assert kind == "mehler" and d <= 2
    return dict(kind="mehler", d=d, t=[0.3, 0.5][:d])


# (kind, N, M, d, noise, S): the first twelve are the cases the nugget rule was tried on in NumPy (SE and Matern 3/2, noise 1e-2 and
# 1e-6, three shapes); the others walk the remaining sizes, dimensions and kernels at the well-conditioned noise
SAMPLER_CASES = [(k, n, m, d, nz, s)
                 for (n, m, d, s) in ((40, 129, 2, 130), (200, 300, 2, 3), (40, 130, 8, 128))
                 for k in ("se", "matern32") for nz in (1e-2, 1e-6)] + [
    ("matern52", 40, 1, 1, 1e-2, 1), ("matern52", 200, 5, 2, 1e-2, 3), ("mehler", 40, 127, 2, 1e-2, 130),
    ("mehler", 40, 128, 1, 1e-2, 1), ("matern52", 40, 128, 8, 1e-2, 128), ("se", 200, 127, 1, 1e-2, 3)]


def case_id(c):
    return "%s-N%d-M%d-d%d-noise%g-S%d" % c


def points_case(kind, n, m, d, noise, seed=0):
    """dict(spec, X (n, d), y (n,), Z (m, d), noise): every Z has z_5 = z_2, z_{M-1} = z_0 and one point ON a training point (as far
    as M allows)."""
    rng = np.random.default_rng(9000 + 13 * n + 7 * m + d + seed)
    X = rng.uniform(-1.0, 1.0, (n, d))
    y = np.sin(2.0 * X.sum(axis=1)) + 0.1 * rng.standard_normal(n)
    Z = rng.uniform(-1.0, 1.0, (m, d))
    if m > 5:
        Z[5] = Z[2]
    if m > 1:
        Z[m - 1] = Z[0]
    Z[1 if m > 2 else 0] = X[3]
    if m == 2:
        Z[1] = Z[0]
    return dict(spec=kernel_spec(kind, d), X=X, y=y, Z=Z, noise=float(noise))


def device_spec(dev, spec):
    """The KernelSpec the device is given for a spec dict."""
    return dev.KernelSpec(P.KIND_ID[spec["kind"]], spec["d"], KR.hyp_of(spec))


def base_samples(s, m, seed=1):
    return np.random.default_rng(seed).standard_normal((s, m))


def cov_f64(spec, A, B=None):
    """K(A, B) in float64 in the per-pair order (Mehler included)."""
    B = A if B is None else B
    return P.mehler_f64(spec, A, B) if spec["kind"] == "mehler" else DR.cov_f64(spec, A, B)


def prior_max(spec, Z):
    return float(np.max(np.diag(cov_f64(spec, Z)))) if spec["kind"] == "mehler" else float(spec["signalSize"])


def host_posterior(c, Z=None):
    """(mean (M,), C (M, M)) of the posterior at Z in float64 NumPy: the stand-in's arithmetic (LAPACK solves)."""
    spec, X, Z = c["spec"], c["X"], c["Z"] if Z is None else Z
    K = cov_f64(spec, X)
    K[np.diag_indices_from(K)] += c["noise"]
    cf = sl.cho_factor(K, lower=True)
    L = np.tril(cf[0])
    Bx = cov_f64(spec, X, Z)
    W = sl.solve_triangular(L, Bx, lower=True)
    kzz = cov_f64(spec, Z)
    Cm = 0.5 * (kzz + kzz.T) - W.T @ W
    return Bx.T @ sl.cho_solve(cf, c["y"]), 0.5 * (Cm + Cm.T)


# ---- references and comparators ---------------------------------------------------------------------------------------------------
def factor_bound(m):
    return CR.MARGIN * (m + 1) * U


def factor_residual(F, Chat):
    """max_ij |F F^T - Chat|_ij / sqrt(Chat_ii Chat_jj), the product in longdouble."""
    F = np.ascontiguousarray(F, dtype=float)
    R = np.abs(np.asarray(Chat, dtype=LD) - CR._ld_matmul(F, np.ascontiguousarray(F.T)))
    dg = np.sqrt(np.diag(Chat).astype(float))
    q = np.asarray(R / (dg[:, None] * dg[None, :]).astype(LD), dtype=float)
    return float(np.max(q)) if np.all(np.isfinite(q)) else float("inf")


def check_factor(F, Chat, label=""):
    """The factor contract: lower triangular EXACTLY, and the backward error under factor_bound(M).  Returns residual / bound."""
    F = np.asarray(F, dtype=float)
    m = F.shape[0]
    assert np.all(np.isfinite(F)), "%s: the factor is not finite" % label
    assert np.all(np.triu(F, 1) == 0.0), "%s: the strict upper triangle of the factor is not exactly 0" % label
    r, b = factor_residual(F, Chat), factor_bound(m)
    print("  %-40s |F F^T - Chat| / sqrt(Chat_ii Chat_jj) = %.3e   bound %g (%d + 1) u = %.3e   ratio %.3f" % (label, r, CR.MARGIN, m, b, r / b))
    assert r <= b, "%s: factor residual %.3e above %g (%d + 1) u = %.3e" % (label, r, CR.MARGIN, m, b)
    return r / b


def draw_replay(mean, F, xi):
    """(S, M) mean + F xi in longdouble."""
    return np.asarray(mean, dtype=LD)[None, :] + CR._ld_matmul(np.ascontiguousarray(xi, dtype=float),
                                                              np.ascontiguousarray(np.asarray(F, dtype=float).T))


def draw_bound(mean, F, xi):
    m = np.asarray(F).shape[0]
    return (m + 2) * U * (np.abs(np.asarray(mean, dtype=float))[None, :] + np.abs(xi) @ np.abs(np.asarray(F, dtype=float)).T)


def check_draw(out, mean, F, xi, label=""):
    """|out - (mean + F xi)| <= draw_bound, everywhere.  Returns the worst error / bound."""
    out = np.asarray(out, dtype=float)
    assert out.shape == np.asarray(xi).shape and np.all(np.isfinite(out)), "%s: shape / finiteness of the samples" % label
    err = np.abs(out.astype(LD) - draw_replay(mean, F, xi))
    bnd = draw_bound(mean, F, xi)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(bnd > 0, np.asarray(err, dtype=float) / bnd, np.where(np.asarray(err, dtype=float) == 0, 0.0, np.inf))
    w = float(np.max(q))
    print("  %-40s worst |draw - replay| / bound = %.3f" % (label, w))
    assert w <= 1.0, "%s: a sample misses its forward bound by a factor %.3g" % (label, w)
    return w


def first_argbest(rows, minimize=True):
    """Per row the FIRST index of the minimum (maximum) among the entries that are not NaN -- np.argmin / np.argmax on a row without
    NaN; a NaN never wins, and a row of nothing but NaN gives index 0 (np.argmin's answer there)."""
    rows = np.asarray(rows, dtype=float)
    nan = np.isnan(rows)
    key = np.where(nan, np.inf, rows if minimize else -rows)
    return np.argmax(~nan & (key == key.min(axis=1)[:, None]), axis=1).astype(np.int64)


def check_argbest_bits(idx, val, rows, minimize=True, label=""):
    """check_argbest for rows that may hold NaN: the indices exactly; the values bit for bit where finite, NaN where NaN."""
    idx, val, rows = np.asarray(idx), np.asarray(val, dtype=float), np.asarray(rows, dtype=float)
    want = first_argbest(rows, minimize)
    assert idx.dtype == np.int64 and np.array_equal(idx, want), "%s: arg-best %r, first arg-best of the rows %r" % (label, idx, want)
    wv = rows[np.arange(rows.shape[0]), want]
    assert np.array_equal(np.isnan(val), np.isnan(wv)), "%s: NaN values %r against %r" % (label, val, wv)
    ok = ~np.isnan(wv)
    assert np.array_equal(val[ok].view(np.int64), wv[ok].view(np.int64)), "%s: values %r against %r" % (label, val, wv)


def check_argbest(idx, val, rows, minimize=True, label=""):
    idx = np.asarray(idx)
    assert idx.dtype == np.int64 and idx.shape == (rows.shape[0],), "%s: indices" % label
    want = first_argbest(rows, minimize)
    assert np.array_equal(idx, want), "%s: not the FIRST arg-%s of the rows (%s)" % (label, "min" if minimize else "max",
                                                                                 np.flatnonzero(idx != want)[:5])
    assert np.array_equal(np.asarray(val), rows[np.arange(rows.shape[0]), want]), "%s: values" % label


def qei_replay(mu, F, xi, fBest, dtype=LD):
    """cost = -(1/S) sum_s max(0, fBest - min_j (mu + F xi_s)_j) in `dtype` from given mu (q,), F (q, q), xi (S, q)."""
    mu, F, xi = np.asarray(mu, dtype=dtype), np.tril(np.asarray(F, dtype=dtype)), np.asarray(xi, dtype=dtype)
    f = mu[None, :] + np.dot(xi, F.T)
    v = np.maximum(dtype(fBest) - np.min(f, axis=1), dtype(0))
    return -(np.sum(v) / dtype(xi.shape[0]))


def qei_bound(mu, F, xi, cost):
    """The bound of the module docstring on |device cost - qei_replay|."""
    mu, F, xi = np.asarray(mu, dtype=float), np.abs(np.tril(np.asarray(F, dtype=float))), np.abs(np.asarray(xi, dtype=float))
    s, q = xi.shape
    a = np.max(np.abs(mu)[None, :] + xi @ F.T, axis=1)
    depth = math.ceil(math.log2(s)) if s > 1 else 0
    return (q + 2) * U * float(np.max(a)) + (depth + 1) * U * abs(float(cost))


def check_qei(cost, mu, F, xi, fBest, label=""):
    ref = qei_replay(mu, F, xi, fBest)
    bnd = qei_bound(mu, F, xi, ref)
    err = abs(float(LD(cost) - ref))
    assert np.isfinite(cost), "%s: cost is not finite" % label
    assert err <= bnd, "%s: cost %.17g misses the replay %.17g by %.3e > bound %.3e" % (label, cost, float(ref), err, bnd)
    return err / bnd


def closed_form_ei(mu, var, fBest):
    """gpx_acq's EI, minimisation form: -s (g Phi(g) + phi(g)), g = (fBest - mu) / s."""
    s = np.sqrt(np.abs(var))
    g = (fBest - mu) / s
    return -s * (g * 0.5 * ssp.erfc(-g / np.sqrt(2.0)) + np.exp(-0.5 * g * g) / np.sqrt(2.0 * np.pi))


def stratified_normal(s):
    """xi_s = Phi^-1((s + 1/2) / S): the midpoint rule in probability."""
    return ssp.ndtri((np.arange(s) + 0.5) / s).reshape(s, 1)


def block_cov_reference(K, Bx, kzz_blocks, q):
    """Per batch b of q consecutive columns of Bx = K(X, Zb): C_b = kzz_b - W_b^T W_b in longdouble with posterior_ref's scale S_c
    restricted to the block (posterior_ref._scales).  Returns (val (B, q, q) longdouble, scale (B, q, q) float64)."""
    Kl = np.asarray(K, dtype=LD)
    L = DR.chol_ld(Kl)
    W = DR.solve_lower_ld(L, np.asarray(Bx, dtype=LD))
    beta = P.solve_upper_ld(L, W)
    nb = Bx.shape[1] // q
    ab, Babs = np.abs(np.asarray(beta, dtype=float)), np.abs(np.asarray(Bx, dtype=float))
    KB = np.abs(np.asarray(K, dtype=float)) @ ab
    val, scale = np.empty((nb, q, q), dtype=LD), np.empty((nb, q, q))
    for b in range(nb):
        sl_ = slice(b * q, (b + 1) * q)
        val[b] = np.asarray(kzz_blocks[b], dtype=LD) - np.dot(W[:, sl_].T, W[:, sl_])
        cross = ab[:, sl_].T @ Babs[:, sl_]
        scale[b] = np.abs(kzz_blocks[b]) + cross + cross.T + ab[:, sl_].T @ KB[:, sl_]
    return val, scale


def block_cov_route(route, K, Bx, kzz_blocks, q):
    """The float64 comparators of posterior_ref (route_values) on the blocks."""
    if route == "lapack":
        L = np.tril(sl.cho_factor(K, lower=True, check_finite=False)[0])
        W = sl.solve_triangular(L, Bx, lower=True, check_finite=False)
    else:
        b = int(route[1:])
        L = CR.chol_block_inverse(K, b)
        W = CR.forward_block_inverse(L, Bx, b)
    nb = Bx.shape[1] // q
    return np.stack([kzz_blocks[b] - W[:, b * q:(b + 1) * q].T @ W[:, b * q:(b + 1) * q] for b in range(nb)])


def block_cov_omega(got, val, scale):
    return P.omega(got, val, scale)


# ---- mutants: each breaks one clause of a contract above ------------------------------------------------------------------------
def mutant_factor_upper_leak(F):
    """A diagonal tile that leaks its upper triangle: one entry above the diagonal left over from C."""
    G = np.array(F, dtype=float)
    G[0, min(1, G.shape[0] - 1)] = G[min(1, G.shape[0] - 1), 0] if G.shape[0] > 1 else G[0, 0]
    return G


def mutant_factor_no_nugget(Cm):
    """chol(C) of the covariance WITHOUT the nugget (judged against C + nugget I); C is shifted just enough to factor."""
    w = np.linalg.eigvalsh(Cm)
    return np.linalg.cholesky(Cm + max(0.0, -2.0 * w[0]) * np.eye(Cm.shape[0]) + 1e-300 * np.eye(Cm.shape[0]))


def mutant_draw_other_row(mean, F, xi):
    """Sample s computed from xi of row s + 1."""
    return np.asarray(draw_replay(mean, F, np.roll(xi, -1, axis=0)), dtype=float)


def mutant_argbest_last(rows, minimize=True):
    r = rows if minimize else -rows
    return (rows.shape[1] - 1 - np.argmin(r[:, ::-1], axis=1)).astype(np.int64)


def mutant_qei_min_after_clamp(mu, F, xi, fBest):
    f = np.asarray(mu)[None, :] + xi @ np.tril(F).T
    return -float(np.mean(np.min(np.maximum(fBest - f, 0.0), axis=1)))


def mutant_qei_short_average(mu, F, xi, fBest):
    f = np.asarray(mu)[None, :] + xi @ np.tril(F).T
    v = np.maximum(fBest - np.min(f, axis=1), 0.0)
    return -float(np.sum(v[:-1]) / xi.shape[0])


# ---- the NumPy stand-in for the new calls of gpexp_amd.device ------------------------------------------------------------------------
class HostFactor(object):
    """What the stand-in takes for a device factor: the lower Cholesky factor of K(X) + noise I on the host."""

    def __init__(self, L):
        self.a = np.asarray(L, dtype=float)


class NumpySampleDevice(object):
    """gpexp_amd.device's new calls (PosteriorSampler, acq_qei) and the few old ones their Python layer reads, on host arrays, from
    the definitions.  The class API's host logic -- shapes, errors, base-sample rules, the session rule -- runs on it unchanged."""
    QEI_MAX_Q = QEI_MAX_Q
    LIE_BELIEVER, LIE_CONSTANT = 0, 1
    ACQ_UCB, ACQ_PI, ACQ_EI = 0, 1, 2
    K_MEHLER = 3

    def __init__(self):
        self.calls = []
        from gpexp_amd import _lib
        self._lib = _lib

    def context(self):
        return self

    def points(self, ctx, x):
        x = np.array(x, dtype=float)
        assert x.ndim == 2
        return x

    @staticmethod
    def spec_dict(spec):
        kind = {0: "se", 1: "matern32", 2: "matern52", 3: "mehler"}[spec.kind]
        hyp, d = np.asarray(spec.hyp, dtype=float), spec.d
        if kind == "se":
            return dict(kind=kind, d=d, cl=list(hyp[:d]), signalSize=float(hyp[d]))
        if kind == "mehler":
            return dict(kind=kind, d=d, t=list(hyp[:d]))
        return dict(kind=kind, d=d, rho=float(hyp[0]), signalSize=float(hyp[1]))

    def kdiag(self, ctx, spec, Z):
        return np.diag(cov_f64(self.spec_dict(spec), Z)).copy()

    def _posterior(self, spec, L, X, alpha, Z):
        s = self.spec_dict(spec)
        kzz = cov_f64(s, Z)
        if L is None:
            return np.zeros(Z.shape[0]), 0.5 * (kzz + kzz.T)
        Bx = cov_f64(s, X, Z)
        W = sl.solve_triangular(np.tril(L.a), Bx, lower=True)
        Cm = kzz - W.T @ W
        return Bx.T @ np.asarray(alpha, dtype=float), 0.5 * (Cm + Cm.T)

    def PosteriorSampler(self, ctx, spec, L, X, alpha, Z, nugget):
        self.calls.append(("psampler", Z.shape[0], float(nugget), L is None))
        mean, Cm = self._posterior(spec, L, X, alpha, Z)
        return _NumpySampler(self, mean, Cm, float(nugget), Z)

    def acq_qei(self, ctx, spec, L, X, alpha, Zb, q, xi, fBest, nugget, want_costs=True):
        self.calls.append(("qei", Zb.shape[0] // q, q, xi.shape, float(fBest), float(nugget)))
        costs, nbad = [], 0
        for b in range(Zb.shape[0] // q):
            mu, Cb = self._posterior(spec, L, X, alpha, Zb[b * q:(b + 1) * q])
            try:
                if nugget == 0.0 and first_repeated_row(Zb[b * q:(b + 1) * q]):
                    raise np.linalg.LinAlgError("pivot 0")
                F = np.linalg.cholesky(Cb + nugget * np.eye(q))
                costs.append(float(qei_replay(mu, F, xi, fBest, dtype=np.float64)))
            except np.linalg.LinAlgError:
                costs.append(float("nan"))
                nbad += 1
        costs = np.array(costs)
        ok = np.flatnonzero(~np.isnan(costs))
        best = int(ok[np.argmin(costs[ok])]) if ok.size else -1
        return best, (costs[best] if best >= 0 else float("nan")), (costs if want_costs else None), nbad


def first_repeated_row(Z):
    """1-based index of the first row of Z that repeats an earlier one exactly, 0 when none does: where the factorisation of a
    posterior covariance WITHOUT a nugget meets its first pivot of exactly 0 in exact arithmetic (LAPACK's rounding may leave it a
    few 1e-17 on either side of 0, so the stand-in decides by the definition)."""
    seen = set()
    for i, row in enumerate(np.asarray(Z, dtype=float)):
        key = row.tobytes()
        if key in seen:
            return i + 1
        seen.add(key)
    return 0


class _NumpySampler(object):
    def __init__(self, be, mean, Cm, nugget, Z):
        self.be, self.mean, self.closed = be, mean, False
        if nugget == 0.0 and first_repeated_row(Z):
            raise be._lib.NotPositiveDefinite(first_repeated_row(Z))
        try:
            self.F = np.linalg.cholesky(Cm + nugget * np.eye(Cm.shape[0]))
        except np.linalg.LinAlgError:
            raise be._lib.NotPositiveDefinite(1)

    def draw(self, xi):
        assert not self.closed and xi.dtype == np.float64 and xi.flags["C_CONTIGUOUS"] and xi.shape[1] == self.mean.size
        return self.mean[None, :] + xi @ self.F.T

    def argbest(self, xi, minimize=True, want_samples=False):
        rows = self.draw(xi)
        idx = first_argbest(rows, minimize)
        val = rows[np.arange(rows.shape[0]), idx]
        return (idx, val, rows) if want_samples else (idx, val)

    def close(self):
        self.closed = True
