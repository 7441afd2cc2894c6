"""CPU-only checks of the cases of tests/grad_dims_cases.py (d = 2, 9, 16, 17, 32), before a kernel is judged by them in
tests/test_gpu_grad_dims.py.

1. Finite differences: every reference gradient of the GPU file is the derivative of the reference VALUE at these dimensions too,
   at the bound of the existing host test of that reference (tests/test_oracle_golden.py, test_loo_host.py,
   test_fitc_grad_host.py, test_fitc_loo_host.py, test_fitc_inducing_host.py, test_vfe_host.py, test_vfe_acq_host.py,
   test_matern_pointgrad_host.py) and at its step, except where the test says why another step serves these cases (the sparse
   gradients: lengths of order sqrt(d) make the derivatives w.r.t. the inducing points small against the cancellation error of
   a difference at 1e-5, and the smallest hyper-gradient entries are 5e-5 of the largest).  Point gradients: 6 points x all d
   coordinates.  The squared exponential's point gradients keep
   the reference's convention, in which the kernel's derivative carries signalSize twice (kernels.py:177): every term of the three
   gradients is linear in that derivative, so they are signalSize times the derivative of the variance, and are held to it at
   the Matern bound.  The FITC point gradients are the same functions with another precision matrix (gp.py:322 differentiates
   K alone, not the FITC precision), so they are no derivative of a value and have no check of their own here.
2. Condition: in every squared-exponential case each of the d length-scale components of a reference gradient is at least 1e-3 of
   the largest of them, so that no length is judged only against another one's size.
3. Sensitivity: the reference with the last two correlation lengths exchanged (squared exponential) or with the last coordinate
   of the evaluation points / candidates zeroed (point gradients) differs from the reference by more than 100 times the bound of
   the GPU test, in the GPU test's metric: a kernel that confuses or drops the last coordinates cannot pass."""
import numpy as np
import pytest

import fitc_grad_ref as fref
import fitc_inducing_ref as iref
import fitc_loo_ref as flref
import grad_dims_cases as gc
import loo_ref
import vfe_acq_ref as aref
import vfe_ref as vref
from helpers import rel
from oracle import gpexp_oracle as orc


def mutated_point_grads(c, Z=None, prec=None):
    """The point gradients of a mutated case: the squared exponential's through the dense algebra (held to the oracle's loops at
    1e-10 below), which spares the oracle's O(N d) Python iterations per mutation."""
    return gc.se_point_grads_dense(c, Z=Z, prec=prec) if c.kind == "se" else gc.point_grads(c, Z=Z, prec=prec)


SE = [p for p in gc.PARAMS if p[0] == "se"]
SE_IDS = ["%s-d%d" % p for p in SE]
H = 1e-5


def theta_of(c):
    return np.concatenate([gc.hyp_of(c.spec), [c.noise]])


def central(value_of, theta, relstep, fourth_order=False):
    """Central differences of value_of(spec hyper-parameters, noise) at the relative step `relstep`; fourth_order: the steps h and
    h / 2 combined as (4 D(h / 2) - D(h)) / 3, which removes the h^2 term of the truncation error."""
    def diff(k, h):
        tp, tm = theta.copy(), theta.copy()
        tp[k] += h
        tm[k] -= h
        return (value_of(tp[:-1], float(tp[-1])) - value_of(tm[:-1], float(tm[-1]))) / (2.0 * h)

    out = np.empty(theta.size)
    for k in range(theta.size):
        h = relstep * theta[k]
        out[k] = (4.0 * diff(k, 0.5 * h) - diff(k, h)) / 3.0 if fourth_order else diff(k, h)
    return out


def drawn_entries(g):
    """Eight entries of a (nu, d) gradient: the largest one, the first one, six drawn (tests/test_fitc_inducing_host.py)."""
    rng = np.random.default_rng(7)
    return [int(np.argmax(np.abs(g))), 0] + [int(v) for v in rng.choice(g.size, 6, replace=False)]


def inducing_fd(c, value_of, g):
    """Worst error of eight entries of dL/dS against central differences, of the largest entry.  The step follows the length
    scales, which the recipe scales with sqrt(d): 1e-4 sqrt(d).  (At 1e-5 the cancellation error of the difference, eps |L| / h with
    |L| of a few hundred, is up to 4e-5 of the largest entry of these gradients, which shrink as the lengths grow.)"""
    worst, h = 0.0, 1e-4 * np.sqrt(c.d)
    for idx in drawn_entries(g):
        u, l = divmod(idx, c.d)
        Sp, Sm = np.array(c.S), np.array(c.S)
        Sp[u, l] += h
        Sm[u, l] -= h
        fd = (value_of(Sp) - value_of(Sm)) / (2.0 * h)
        worst = max(worst, abs(fd - g[u, l]) / np.max(np.abs(g)))
    return worst


# ---- 1. finite differences ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,d", gc.PARAMS, ids=gc.IDS)
def test_dense_likelihood_gradients_match_central_differences(kind, d):
    """oracle.loglike_grad against oracle.loglike (2e-6 per entry: tests/test_oracle_golden.py); loo_ref's closed form against
    loo_ref.loo_grad_fd (h = 1e-5, 1e-5 of the largest entry: tests/test_loo_host.py)."""
    c = gc.case(kind, d)
    theta = theta_of(c)
    value, g = gc.reference(kind, d, "lml")
    assert value == pytest.approx(orc.loglike(c.spec, c.X, c.y, c.noise), rel=1e-12)
    fd = central(lambda hyp, nz: orc.loglike(fref.spec_with(c.spec, hyp), c.X, c.y, nz), theta, 1e-5)
    e_lml = gc.entry_relerr(g, fd)
    # the oracle's pinv form against the Cholesky form: well inside a tenth of the device test's 1e-9 per entry (seen <= 1.2e-12)
    assert gc.entry_relerr(gc.lml_other(c), g) <= 1e-10
    g_loo = gc.reference(kind, d, "loo")[3]
    e_loo = gc.max_relerr(g_loo, loo_ref.loo_grad_fd(gc.LOO_KIND[kind], d, gc.hyp_of(c.spec), c.X, c.noise, c.y, h=H))
    print("%s d=%d: log-marginal %.2e per entry, leave-one-out %.2e of the largest" % (kind, d, e_lml, e_loo))
    assert g.shape == g_loo.shape == theta.shape
    assert e_lml <= 2e-6, (g, fd)
    assert e_loo <= 1e-5


@pytest.mark.parametrize("kind,d", gc.PARAMS, ids=gc.IDS)
def test_sparse_gradients_match_central_differences(kind, d):
    """FITC likelihood (oracle.fitc_loglike, 1e-6 per entry), FITC leave-one-out (dense value, 1e-5 theta, 1e-6 of the largest), VFE
    bound (1e-6 per entry), dL/dS and dF/dS (eight entries, 1e-5 of the largest): the bounds of the existing host tests.  The two
    per-entry comparisons use fourth-order central differences at the relative step 8e-3: the smallest entries here are 5e-5 of
    the largest, and at second order no step serves them -- at 1e-4 the cancellation error alone is up to 6e-6 of such an entry, at
    1e-3 the truncation error 5e-5 (measured).  At fourth order the error still falls as the step grows from 1e-3 to 8e-3 (it is
    the cancellation of the value, eighty times smaller than at 1e-4); seen <= 6.2e-7."""
    c = gc.case(kind, d)
    theta = theta_of(c)
    cond = fref.cond_quu(c.spec, c.S, c.noise)
    assert cond <= 1e4, cond
    value, g = gc.reference(kind, d, "fitc_lml")
    # (the oracle inverts g + 1e-12, gp.py:200: that moves sum log g by up to N 1e-12 / noise, which the restatement leaves out)
    assert abs(value - orc.fitc_loglike(c.spec, c.X, c.y, c.noise, c.S)) <= 1e-10 * abs(value) + gc.N * 1e-12 / c.noise
    errs = {"fitc_lml": gc.entry_relerr(g, central(lambda hyp, nz: orc.fitc_loglike(fref.spec_with(c.spec, hyp), c.X, c.y, nz, c.S), theta, 8e-3,
                                                   fourth_order=True))}
    g = gc.reference(kind, d, "fitc_loo")["grad"]
    errs["fitc_loo"] = gc.max_relerr(central(lambda hyp, nz: flref.dense_value(fref.spec_with(c.spec, hyp), c.X, c.S, c.y, nz), theta, 1e-5), g)
    _, g, gs = gc.reference(kind, d, "vfe")
    errs["vfe"] = gc.entry_relerr(g, central(lambda hyp, nz: vref.value(fref.spec_with(c.spec, hyp), c.X, c.S, c.y, nz), theta, 8e-3,
                                             fourth_order=True))
    errs["vfe_inducing"] = inducing_fd(c, lambda S: vref.value(c.spec, c.X, S, c.y, c.noise), gs)
    errs["fitc_inducing"] = inducing_fd(c, lambda S: iref.value(c.spec, c.X, S, c.y, c.noise), gc.reference(kind, d, "fitc_inducing"))
    print("%s d=%d: cond(Quu) %.1e  " % (kind, d, cond) + "  ".join("%s %.2e" % kv for kv in errs.items()))
    assert errs["fitc_lml"] <= 1e-6 and errs["fitc_loo"] <= 1e-6 and errs["vfe"] <= 1e-6, errs
    assert errs["vfe_inducing"] <= 1e-5 and errs["fitc_inducing"] <= 1e-5, errs


@pytest.mark.parametrize("kind,d", gc.PARAMS, ids=gc.IDS)
def test_point_gradients_match_central_differences_of_the_variance(kind, d):
    """6 evaluation points (d var / d z) and 6 training points (d var(z_m) / d x_j for every m, and the IVAR gradient) x all d
    coordinates, h = 1e-5, 2e-6 of the largest entry of the subset (tests/test_matern_pointgrad_host.py).  The differences over the
    refits are taken of the dense-algebra variance, held to oracle.posterior's first."""
    c = gc.case(kind, d)
    full, newpt, ivar = gc.reference(kind, d, "point")
    scale = c.spec["signalSize"] if kind == "se" else 1.0      # the reference's doubled signalSize (module docstring)
    v0 = gc.variance(c, c.X, c.Z)
    assert np.all(v0 > 0.0) and rel(gc.variance_dense(c, c.X, c.Z), v0) <= 1e-10
    pts = list(gc.FD_POINTS)
    Zs = np.array(c.Z[pts])
    fd_new = np.empty((len(pts), d))
    for l in range(d):
        Zp, Zm = Zs.copy(), Zs.copy()
        Zp[:, l] += H
        Zm[:, l] -= H
        fd_new[:, l] = (gc.variance_dense(c, c.X, Zp) - gc.variance_dense(c, c.X, Zm)) / (2.0 * H)
    rows = np.array([j * d + l for j in pts for l in range(d)])
    fd_full = np.empty((rows.size, gc.M))
    for r, (j, l) in enumerate((j, l) for j in pts for l in range(d)):
        Xp, Xm = np.array(c.X), np.array(c.X)
        Xp[j, l] += H
        Xm[j, l] -= H
        fd_full[r] = (gc.variance_dense(c, Xp, c.Z) - gc.variance_dense(c, Xm, c.Z)) / (2.0 * H)
    errs = (rel(newpt.reshape(gc.M, d)[pts], scale * fd_new), rel(full[rows], scale * fd_full),
            rel(ivar[rows], scale * fd_full.mean(axis=1)))
    print("%s d=%d: newpt %.2e  full %.2e  ivar %.2e" % ((kind, d) + errs))
    assert full.shape == (gc.N * d, gc.M) and newpt.shape == (gc.M * d,) and ivar.shape == (gc.N * d,)
    assert max(errs) <= 2e-6, errs
    if kind == "se":   # the oracle's loops and the dense algebra: the two forms of the squared exponential's gradients
        other = gc.se_point_grads_dense(c)
        assert max(rel(a, b) for a, b in zip(other, (full, newpt, ivar))) <= 1e-10


@pytest.mark.parametrize("kind,d", gc.PARAMS, ids=gc.IDS)
def test_acquisition_gradients_match_central_differences(kind, d):
    """The closed forms of bo_compose.DenseModel.grad and vfe_acq_ref at 6 candidates x all d coordinates: h = 1e-5, 1e-6 of the
    largest entry (tests/test_vfe_acq_host.py, tests/test_gpu_bo.py); the VFE form in its two summation orders to 1e-10.  A
    difference of costs resolves eps / h = 1e-11: where PI or EI with fBest = max y is so far in the tail that no difference
    reaches 1e-3 (grad_dims_cases.ACQ) the figure is printed only, and the same cost with fBest = median y carries the check."""
    c = gc.case(kind, d)
    pts = list(gc.FD_POINTS)
    Cs = np.array(c.C[pts])
    dense, sparse = gc.reference(kind, d, "acq"), gc.reference(kind, d, "vfe_acq")
    other = gc.vfe_acq_grads(c, reordered=True)
    for name in gc.ACQS:
        fd = aref.central_differences(lambda P: gc.acq_costs(c, name, P), Cs, h=H)
        fd_v = aref.central_differences(lambda P: gc.vfe_acq_costs(c, name, P), Cs, h=H)
        e, e_v = gc.max_relerr(dense[name][pts], fd), gc.max_relerr(sparse[name][pts], fd_v)
        e_o = gc.max_relerr(sparse[name], other[name])
        print("%s d=%d %s: dense %.2e  VFE %.2e  VFE, two summation orders %.2e" % (kind, d, name, e, e_v, e_o))
        assert dense[name].shape == sparse[name].shape == (gc.M, d)
        assert e_o <= 1e-10, (name, e_o)
        for err, diffs in ((e, fd), (e_v, fd_v)):
            resolved = np.max(np.abs(diffs)) > 1e-3
            assert resolved or name in ("pi", "ei"), (name, np.max(np.abs(diffs)))
            assert err <= 1e-6 or not resolved, (name, err)


# ---- 2. condition ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,d", SE, ids=SE_IDS)
def test_every_length_scale_component_is_within_three_decades_of_the_largest(kind, d):
    grads = {"lml": gc.reference(kind, d, "lml")[1], "loo": gc.reference(kind, d, "loo")[3], "fitc_lml": gc.reference(kind, d, "fitc_lml")[1],
             "fitc_loo": gc.reference(kind, d, "fitc_loo")["grad"], "vfe": gc.reference(kind, d, "vfe")[1]}
    for what, g in grads.items():
        lengths = np.abs(g[:d])
        print("%s d=%d %s: smallest / largest length-scale component %.2e" % (kind, d, what, lengths.min() / lengths.max()))
        assert g.shape == (d + 2,) and lengths.min() >= 1e-3 * lengths.max(), (what, g)


# ---- 3. sensitivity ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,d", SE, ids=SE_IDS)
def test_exchanging_the_last_two_lengths_shows_in_every_reference(kind, d):
    c = gc.case(kind, d)
    s = gc.swapped(c)
    assert s.spec["cl"][d - 1] == c.spec["cl"][d - 2] != c.spec["cl"][d - 1]
    got = {"lml": (gc.lml(s)[1], gc.reference(kind, d, "lml")[1]), "loo": (gc.loo(s)[3], gc.reference(kind, d, "loo")[3]),
           "fitc_lml": (gc.fitc_lml(s)[1], gc.reference(kind, d, "fitc_lml")[1]),
           "fitc_loo": (gc.fitc_loo(s)["grad"], gc.reference(kind, d, "fitc_loo")["grad"]),
           "fitc_inducing": (gc.fitc_inducing(s), gc.reference(kind, d, "fitc_inducing")),
           "vfe": (gc.vfe(s)[1], gc.reference(kind, d, "vfe")[1]), "vfe_inducing": (gc.vfe(s)[2], gc.reference(kind, d, "vfe")[2])}
    dense, sparse = mutated_point_grads(s), mutated_point_grads(s, prec=gc.fitc_prec(s))
    for i, name in enumerate(("point_full", "point_newpt", "point_ivar")):
        got[name] = (dense[i], gc.reference(kind, d, "point")[i])
        got["fitc_" + name] = (sparse[i], gc.reference(kind, d, "fitc_point")[i])
    for name in gc.ACQS:
        got["acq_" + name] = (gc.acq_grads(s)[name], gc.reference(kind, d, "acq")[name])
        got["vfe_acq_" + name] = (gc.vfe_acq_grads(s)[name], gc.reference(kind, d, "vfe_acq")[name])
    for name, (mutated, ref) in got.items():
        what = next(w for w in sorted(gc.TOL, key=len, reverse=True) if name.startswith(w))
        e = gc.err(what, mutated, ref)
        print("%s d=%d %s: %.2e = %.1e x the bound" % (kind, d, name, e, e / gc.TOL[what][1]))
        assert e > 100.0 * gc.TOL[what][1], (name, e)


@pytest.mark.parametrize("kind,d", gc.PARAMS, ids=gc.IDS)
def test_zeroing_the_last_coordinate_of_the_evaluation_points_shows_in_every_point_gradient(kind, d):
    c = gc.case(kind, d)
    # once per case: the two NumPy forms of the FITC reference against each other, in the GPU test's metric
    gap = gc.fitc_point_gap(c)
    print("%s d=%d FITC point gradients against the Cholesky-solve form: explicit Woodbury precision %.2e, oracle.fitc_matrices %.2e" % ((kind, d) + gap))
    assert gap[0] <= 0.1 * gc.TOL["fitc_point"][1]
    P = gc.fitc_prec(c)
    Z0, C0 = gc.zeroed(c.Z), gc.zeroed(c.C)
    got = {}
    dense, sparse = mutated_point_grads(c, Z=Z0), mutated_point_grads(c, Z=Z0, prec=P)
    for i, name in enumerate(("point_full", "point_newpt", "point_ivar")):
        got[name] = (dense[i], gc.reference(kind, d, "point")[i])
        got["fitc_" + name] = (sparse[i], gc.reference(kind, d, "fitc_point")[i])
    for name in gc.ACQS:
        got["acq_" + name] = (gc.acq_grads(c, C=C0)[name], gc.reference(kind, d, "acq")[name])
        got["vfe_acq_" + name] = (gc.vfe_acq_grads(c, C=C0)[name], gc.reference(kind, d, "vfe_acq")[name])
    for name, (mutated, ref) in got.items():
        what = next(w for w in sorted(gc.TOL, key=len, reverse=True) if name.startswith(w))
        e = gc.err(what, mutated, ref)
        print("%s d=%d %s: %.2e = %.1e x the bound" % (kind, d, name, e, e / gc.TOL[what][1]))
        assert e > 100.0 * gc.TOL[what][1], (name, e)
