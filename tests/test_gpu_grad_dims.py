"""Every gradient entry point of the device over the dimension classes up to 32 (-m gpu): the cases of tests/grad_dims_cases.py
(N = 300, 70 evaluation points / candidates / inducing points; squared exponential with d distinct lengths, Matern 3/2 and 5/2)
through the gpexp_amd.device wrapper, against the NumPy reference, with the metric and the bound of the existing parity test of
the same entry point (grad_dims_cases.TOL).  tests/test_grad_dims_host.py ties every reference to central differences at these
dimensions and shows that exchanging or dropping the last coordinates moves each of them by more than 100 bounds.

    entry point (device wrapper)                                      d                 what the dimension selects
    gpx_lml_grad, _linv, _rows, _slab                                 2, 9, 16, 17, 32  partial stride nd + 2 = 4 .. 34, LDS 2 * 64 * d doubles,
                                                                                        a final reduction of 34 blocks (squared exponential)
    gpx_loo_grad (slab_rows 0, 128, 256)                              2, 9, 16, 17, 32  loo_dkfill_kernel: LDS 2 * 64 * d, one fill per length
    gpx_var_grad                                                      2, 9, 16, 17, 32  dcov_kernel / var_grad_finish_kernel, one product per coordinate
    gpx_var_grad_newpt                                                2, 9, 16, 17, 32  var_grad_newpt_radial_kernel<KIND, 2 | 16 | 32>
    gpx_ivar_grad_w (plain, W=), gpx_ivar_grad_rows (r0 = 128, 256)   2, 9, 16, 17, 32  ivar_grad_row_radial_kernel<KIND, 2 | 16 | 32>, radial_finish
    gpx_fitc_var_grad, gpx_fitc_var_grad_newpt                        2, 9, 16, 17, 32  the same kernels behind the Woodbury precision
    gpx_acq_grad (UCB, PI, EI)                                        2, 9, 16, 17, 32  acq_grad_kernel<KIND, 2 | 16 | 32, false>
    gpx_vfe_acq_grad (UCB, PI, EI)                                    2, 9, 16, 17, 32  acq_grad_kernel<KIND, 2 | 16 | 32, true>
    gpx_fitc_lml_grad, gpx_fitc_loo_grad, gpx_vfe_grad (hyper)        2, 9, 16, 17, 32  fitc_wsum_kernel: partial stride nd + 1 = 3 .. 33, LDS 2 * 64 * d
    gpx_fitc_lml_grad_inducing, gpx_vfe_grad (inducing)               2, 9, 16, 17, 32  fitc_wgrad_kernel<KIND, 2 | 16 | 32>: 1, 4 or 8 passes per strip
    embedding d -> d + 1                                              8 -> 9, 16 -> 17  the arrays of 8 | 16 | 32 against each other
    class API (loglikeParams, looLogLike, derivativeBatch)            17                keys cl0 .. cl16

(Matern kernels have one length: their hyper-parameter entries take the nd = 1 strides at every d, and d enters through the LDS
staging and the distance loops.)

Seen on an MI355X, the worst of the three kernels, in the metric of the bound:

    entry point                               bound   d = 2     9         16        17        32
    lml_grad, every form                      1e-9    2.2e-13   1.1e-12   1.7e-13   1.1e-12   1.9e-13   (forms among each other <= 9.2e-14)
    loo_grad, every slab size                 1e-9    7.6e-15   1.8e-13   1.1e-13   7.3e-14   3.1e-14
    var_grad                                  1e-9    4.8e-12   3.0e-12   1.1e-12   1.6e-12   7.2e-13
    var_grad_newpt                            1e-9    1.1e-11   2.3e-12   1.1e-12   1.1e-12   4.8e-13
    ivar_grad (plain, W=), ivar_grad_rows     1e-9    4.0e-12   3.6e-12   1.8e-12   5.1e-12   1.0e-12
    fitc var_grad, var_grad_newpt             1e-8    9.5e-11   2.2e-10   2.3e-10   1.5e-10   9.1e-11
    acq_grad                                  1e-9    6.0e-12   3.8e-12   1.9e-12   9.7e-13   5.7e-13
    vfe acq_grad                              1e-8    7.7e-9    5.3e-9    3.5e-10   9.1e-11   3.6e-10   (PI, fBest = max y: in the tail)
    fitc lml_grad                             1e-8    2.0e-10   2.2e-10   7.5e-11   4.8e-11   6.1e-11
    fitc lml_grad, inducing points            1e-8    7.4e-11   6.4e-11   4.9e-11   5.3e-11   3.8e-11
    fitc loo_grad                             1e-8    1.1e-10   1.6e-9    3.0e-10   1.8e-10   2.0e-10
    vfe grad                                  1e-8    9.8e-11   1.1e-9    9.6e-10   5.4e-11   3.5e-11
    vfe grad, inducing points                 1e-8    5.1e-11   5.6e-11   5.2e-11   3.9e-11   3.0e-11
    embedding 8 -> 9 and 16 -> 17             as above: every gradient equal bit for bit, the extra component exactly 0

No bound was re-derived: the one reference whose NumPy forms differ by more than a tenth of its bound, the FITC point gradients
through oracle.fitc_matrices, has a form that does not (test_point_gradients_of_the_variance_on_a_fitc_model)."""
import numpy as np
import pytest

import fitc_grad_ref as fref
import grad_dims_cases as gc

pytestmark = pytest.mark.gpu

EMBED = [(kind, d) for kind in ("se", "matern52") for d in (8, 16)]
EMBED_IDS = ["%s-d%d-d%d" % (k, d, d + 1) for k, d in EMBED]


def kernel_spec(dev, c):
    return dev.KernelSpec(fref.KIND_ID[c.kind], c.d, gc.hyp_of(c.spec))


def dense_model(c):
    """(dev, ctx, ks, Xd, L, alpha): the factor of K(X, X) + noise I and alpha = K^-1 y."""
    from gpexp_amd import device as dev
    ctx = dev.context()
    ks = kernel_spec(dev, c)
    Xd = dev.points(ctx, c.X)
    L = dev.potrf(ctx, dev.kfill(ctx, ks, Xd, nugget=c.noise))
    return dev, ctx, ks, Xd, L, dev.potrs(ctx, L, c.y)


def sparse_model(c, cls):
    """(dev, ctx, ks, model) for cls = "FitcModel" | "VfeModel" on (X, S)."""
    from gpexp_amd import device as dev
    ctx = dev.context()
    ks = kernel_spec(dev, c)
    return dev, ctx, ks, getattr(dev, cls)(ctx, ks, dev.points(ctx, c.X), dev.points(ctx, c.S), c.noise)


def held(what, got, ref, label, bound=None):
    """Print the error of `got` in the metric of the entry point's parity test, then hold it to that test's bound."""
    e = gc.err(what, got, ref)
    bound = gc.TOL[what][1] if bound is None else bound
    print("%s: %.2e (%s, bound %.0e)" % (label, e, gc.TOL[what][0], bound))
    assert np.shape(got) == np.shape(ref), label
    assert e <= bound, (label, e)
    return e


# ---- dense model: hyper-parameter gradients --------------------------------------------------------------------------------------
def lml_forms(dev, ctx, ks, Xd, L, alpha, n, monkeypatch):
    """{form: gradient [lengths..., signalSize, noise]} through every form of the trace the library has."""
    npad = (n + 127) // 128 * 128
    forms = {"full": dev.lml_grad_full(ctx, ks, L, Xd, alpha), "linv": dev.lml_grad_from_sums(ks, dev.lml_grad_linv(ctx, ks, L, Xd, alpha)),
             "lml_grad(slabs=3)": dev.lml_grad(ctx, ks, L, Xd, alpha, slabs=3)}
    monkeypatch.setenv("GPX_LML_GRAD_FORM", "slabs")      # neither "linv" nor "rows": the slab loop itself
    forms["slab loop of 3"] = dev.lml_grad(ctx, ks, L, Xd, alpha, slabs=3)
    monkeypatch.delenv("GPX_LML_GRAD_FORM")
    rb = dev.lml_grad_rows_bounds(n, 3)
    assert rb[0] == 0 and rb[-1] == npad and sum(1 for a, b in zip(rb[:-1], rb[1:]) if b > a) >= 2
    forms["rows in ranges"] = dev.lml_grad_from_sums(ks, sum(dev.lml_grad_rows(ctx, ks, L, Xd, alpha, a, b) for a, b in zip(rb[:-1], rb[1:]) if b > a))
    forms["rows, 2 sub-slabs"] = dev.lml_grad_from_sums(ks, dev.lml_grad_rows(ctx, ks, L, Xd, alpha, 0, npad, 2))
    return forms


@pytest.mark.parametrize("kind,d", gc.PARAMS, ids=gc.IDS)
def test_log_marginal_gradient_in_every_form(kind, d, monkeypatch):
    """oracle.loglike_grad, every component to 1e-9 of its own size (tests/test_gpu_api.py, tests/test_gpu_golden_r6.py); the forms
    agree with each other to the same bound."""
    c = gc.case(kind, d)
    ref = gc.reference(kind, d, "lml")[1]
    dev, ctx, ks, Xd, L, alpha = dense_model(c)
    forms = lml_forms(dev, ctx, ks, Xd, L, alpha, gc.N, monkeypatch)
    for name, g in forms.items():
        held("lml", g, ref, "%s d=%d %s" % (kind, d, name))
    for name, g in forms.items():
        held("lml", g, forms["full"], "%s d=%d %s against full" % (kind, d, name))


@pytest.mark.parametrize("kind,d", gc.PARAMS, ids=gc.IDS)
def test_leave_one_out_gradient(kind, d):
    """loo_ref's closed form, 1e-9 of the largest entry (tests/test_gpu_loo.py): the whole matrix at once, and in row slabs of 128
    (three, the last one of 44 rows) and of 256 (two)."""
    c = gc.case(kind, d)
    _, _, l0, g0 = gc.reference(kind, d, "loo")
    dev, ctx, ks, Xd, L, _ = dense_model(c)
    for slab_rows in (0, 128, 256):
        lp, g = dev.loo_grad(ctx, ks, L, Xd, c.noise, c.y, slab_rows=slab_rows)
        held("loo", g, g0, "%s d=%d slab_rows=%d" % (kind, d, slab_rows))
        assert abs(lp - l0) <= 1e-9 * abs(l0)


# ---- dense model: point gradients ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,d", gc.PARAMS, ids=gc.IDS)
def test_point_gradients_of_the_variance(kind, d):
    """The oracle's reference-convention forms (squared exponential) and matern_pointgrad_ref.gradients (Matern), 1e-9 of the
    largest entry (tests/test_gpu_f1.py, tests/test_gpu_matern_pointgrad.py): the (N d, M) matrix, the gradient w.r.t. the
    evaluation points, and the IVAR gradient -- stand-alone, from a kept forward solve, and for the rows from 128 and from 256 on."""
    c = gc.case(kind, d)
    full, newpt, ivar = gc.reference(kind, d, "point")
    dev, ctx, ks, Xd, L, _ = dense_model(c)
    Zd = dev.points(ctx, c.Z)
    tag = "%s d=%d " % (kind, d)
    held("point", dev.var_grad(ctx, ks, L, Xd, Zd), full, tag + "var_grad")
    held("point", dev.var_grad_newpt(ctx, ks, L, Xd, Zd), newpt, tag + "var_grad_newpt")
    held("point", dev.ivar_grad(ctx, ks, L, Xd, Zd), ivar, tag + "ivar_grad")
    cost, W = dev.ivar(ctx, ks, L, Xd, Zd, keep=True)
    assert W is not None and abs(abs(cost) - np.mean(gc.variance(c, c.X, c.Z))) <= 1e-10 * abs(cost)
    held("point", dev.ivar_grad(ctx, ks, L, Xd, Zd, W=W), ivar, tag + "ivar_grad(W=)")
    for r0 in (128, 256):
        held("point", dev.ivar_grad_rows(ctx, ks, L, Xd, Zd, W, r0), ivar[r0 * d:], tag + "ivar_grad_rows(r0=%d)" % r0)


@pytest.mark.parametrize("kind,d", gc.PARAMS, ids=gc.IDS)
def test_point_gradients_of_the_variance_on_a_fitc_model(kind, d):
    """The same references with the precision of the FITC model handed in (`prec=` / the oracle's model dict), 1e-8 of the largest
    entry (tests/test_gpu_matern_pointgrad.py::test_fitc_model, tests/test_gpu_f1.py::test_ivar_cost_with_fitc_model).  The
    precision is grad_dims_cases.FitcSolve, Cholesky solves with the dense Q + G.  Two NumPy forms of this reference: against the
    explicit Woodbury matrix from the model's two factors it moves by <= 1.5e-10 at every case (tests/test_grad_dims_host.py asserts
    a tenth of the bound), so the bound stands.  oracle.fitc_matrices (pinv(Quu) and an explicit inverse of Quu + Kuf G^-1 Kfu) is
    up to 2.1e-6 away from both (matern52 d = 2; 1.3e-6 se d = 2) and is not used; the device was seen that far from it too."""
    c = gc.case(kind, d)
    full, newpt, ivar = gc.reference(kind, d, "fitc_point")
    dev, ctx, ks, model = sparse_model(c, "FitcModel")
    Zd = dev.points(ctx, c.Z)
    got = model.var_grad(ks, Zd)
    held("fitc_point", got, full, "%s d=%d fitc var_grad" % (kind, d))
    held("fitc_point", got.sum(axis=1) / gc.M, ivar, "%s d=%d fitc var_grad, column mean" % (kind, d))
    held("fitc_point", model.var_grad_newpt(ks, Zd), newpt, "%s d=%d fitc var_grad_newpt" % (kind, d))


# ---- acquisition gradients ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,d", gc.PARAMS, ids=gc.IDS)
def test_acquisition_gradients(kind, d):
    """UCB (kappa = 2), PI and EI (fBest = max y) at the 70 candidates: bo_compose.DenseModel.grad to 1e-9 of the largest entry on
    the dense model (tests/test_gpu_bo.py), vfe_acq_ref.grad to 1e-8 on the VFE model (tests/test_gpu_vfe_acq.py)."""
    c = gc.case(kind, d)
    dev, ctx, ks, Xd, L, alpha = dense_model(c)
    Cd = dev.points(ctx, c.C)
    vfe = sparse_model(c, "VfeModel")[3]
    coeff = vfe.solve(c.y)[0]
    for name in gc.ACQS:
        p = gc.acq_param(name, c.y)
        costs, G = dev.acq_grad(ctx, ks, L, Xd, alpha, Cd, gc.ACQ_ID[name], p)
        held("acq", G, gc.reference(kind, d, "acq")[name], "%s d=%d %s dense" % (kind, d, name))
        assert gc.max_relerr(costs, gc.acq_costs(c, name, c.C)) < 1e-10
        costs, G = vfe.acq_grad(coeff, Cd, gc.ACQ_ID[name], p)
        held("vfe_acq", G, gc.reference(kind, d, "vfe_acq")[name], "%s d=%d %s VFE" % (kind, d, name))
        assert gc.max_relerr(costs, gc.vfe_acq_costs(c, name, c.C)) <= 1e-8


# ---- sparse models: hyper-parameter and inducing-point gradients ---------------------------------------------------------------
@pytest.mark.parametrize("kind,d", gc.PARAMS, ids=gc.IDS)
def test_fitc_likelihood_and_leave_one_out_gradients(kind, d):
    """fitc_grad_ref, fitc_inducing_ref and fitc_loo_ref: values 1e-10, every hyper-gradient entry 1e-8 of its own size, dL/dS 1e-8 of
    its largest entry, the leave-one-out mean 1e-8 of the largest and every variance 1e-8 (tests/test_gpu_fitc_grad.py,
    test_gpu_fitc_inducing.py, test_gpu_fitc_loo.py)."""
    c = gc.case(kind, d)
    value, grad = gc.reference(kind, d, "fitc_lml")
    want = gc.reference(kind, d, "fitc_loo")
    dev, ctx, ks, model = sparse_model(c, "FitcModel")
    tag = "%s d=%d " % (kind, d)
    lp0, g0 = model.lml_grad(ks, c.y)
    lp, g, gs = model.lml_grad(ks, c.y, want_inducing=True)
    assert lp == lp0 and np.array_equal(g, g0) and np.all(np.isfinite(gs))
    assert abs(lp - value) <= 1e-10 * abs(value)
    held("fitc_lml", g, grad, tag + "fitc lml_grad")
    held("fitc_inducing", gs, gc.reference(kind, d, "fitc_inducing"), tag + "fitc lml_grad, inducing points")
    mean, var, ll = model.loo(c.y)
    ll2, gl = model.loo_grad(ks, c.y)
    assert ll2 == ll and abs(ll - want["value"]) <= 1e-10 * abs(want["value"])
    assert gc.max_relerr(mean, want["mean"]) <= 1e-8 and gc.entry_relerr(var, want["var"]) <= 1e-8
    held("fitc_loo", gl, want["grad"], tag + "fitc loo_grad")


@pytest.mark.parametrize("kind,d", gc.PARAMS, ids=gc.IDS)
def test_vfe_gradients(kind, d):
    """vfe_ref: F to 1e-10, every hyper-gradient entry 1e-8 of its own size, dF/dS 1e-8 of its largest entry (tests/test_gpu_vfe.py)."""
    c = gc.case(kind, d)
    value, grad, gs_ref = gc.reference(kind, d, "vfe")
    dev, ctx, ks, model = sparse_model(c, "VfeModel")
    lp, g, gs = model.grad(ks, c.y, want_inducing=True)
    assert lp == model.bound(c.y) and abs(lp - value) <= 1e-10 * abs(value) and np.all(np.isfinite(gs))
    held("vfe", g, grad, "%s d=%d vfe grad" % (kind, d))
    held("vfe_inducing", gs, gs_ref, "%s d=%d vfe grad, inducing points" % (kind, d))


# ---- embedding ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,d", EMBED, ids=EMBED_IDS)
def test_a_constant_extra_coordinate_changes_nothing(kind, d, monkeypatch):
    """The model in d coordinates and the same model with one more coordinate, the same constant for every point (length 1 for the
    squared exponential): the same gradient in the first d components, to the bound of the parity assertion, and 0 in the extra one
    -- the coordinate differences there are exactly 0.  d = 8 -> 9 and 16 -> 17 cross from one register-array size to the next, so
    the instantiations of 8, 16 and 32 coordinates are held against each other with no reference in between."""
    c = gc.case(kind, d)
    e = gc.embedded(c)
    nl = d if kind == "se" else 1                            # length-type hyper-parameters of the small model
    tag = "%s d=%d->%d " % (kind, d, d + 1)

    def hyper(g):
        """the large model's gradient without its extra length; that entry"""
        g = np.asarray(g)
        return (np.delete(g, d), g[d]) if kind == "se" else (g, 0.0)

    def points(G):
        """the large model's (rows, d + 1) point gradient without its extra column; that column"""
        G = np.asarray(G).reshape(-1, d + 1)
        return G[:, :d], G[:, d]

    small, large = dense_model(c), dense_model(e)
    dev, ctx = small[0], small[1]
    # one dense hyper gradient, in every form
    fs, fl = (lml_forms(dev, ctx, m[2], m[3], m[4], m[5], gc.N, monkeypatch) for m in (small, large))
    for name in fs:
        body, extra = hyper(fl[name])
        held("lml", body, fs[name], tag + "lml " + name)
        assert extra == 0.0, (name, extra)
    assert len(fs["full"]) == nl + 2
    # dense point gradients
    Zs, Zl = dev.points(ctx, c.Z), dev.points(ctx, e.Z)
    for fn in (dev.var_grad_newpt, dev.ivar_grad):
        body, extra = points(fn(ctx, large[2], large[4], large[3], Zl))
        held("point", body, np.asarray(fn(ctx, small[2], small[4], small[3], Zs)).reshape(-1, d), tag + fn.__name__)
        assert np.all(extra == 0.0), fn.__name__
    full_l = dev.var_grad(ctx, large[2], large[4], large[3], Zl).reshape(gc.N, d + 1, gc.M)
    held("point", full_l[:, :d, :].reshape(gc.N * d, gc.M), dev.var_grad(ctx, small[2], small[4], small[3], Zs), tag + "var_grad")
    assert np.all(full_l[:, d, :] == 0.0)
    # acquisition gradients, dense and VFE
    Cs, Cl = dev.points(ctx, c.C), dev.points(ctx, e.C)
    vs, vl = sparse_model(c, "VfeModel")[3], sparse_model(e, "VfeModel")[3]
    cs, cl = vs.solve(c.y)[0], vl.solve(e.y)[0]
    for name in gc.ACQS:
        p = gc.acq_param(name, c.y)
        k0, G0 = dev.acq_grad(ctx, small[2], small[4], small[3], small[5], Cs, gc.ACQ_ID[name], p)
        k1, G1 = dev.acq_grad(ctx, large[2], large[4], large[3], large[5], Cl, gc.ACQ_ID[name], p)
        held("acq", G1[:, :d], G0, tag + "acq_grad " + name)
        assert np.all(G1[:, d] == 0.0) and gc.max_relerr(k1, k0) < 1e-10
        k0, G0 = vs.acq_grad(cs, Cs, gc.ACQ_ID[name], p)
        k1, G1 = vl.acq_grad(cl, Cl, gc.ACQ_ID[name], p)
        held("vfe_acq", G1[:, :d], G0, tag + "vfe acq_grad " + name)
        assert np.all(G1[:, d] == 0.0) and gc.max_relerr(k1, k0) <= 1e-8
    # FITC likelihood: hyper-parameters and inducing points
    ms, ml = sparse_model(c, "FitcModel"), sparse_model(e, "FitcModel")
    lp0, g0, gs0 = ms[3].lml_grad(ms[2], c.y, want_inducing=True)
    lp1, g1, gs1 = ml[3].lml_grad(ml[2], e.y, want_inducing=True)
    body, extra = hyper(g1)
    assert abs(lp1 - lp0) <= 1e-10 * abs(lp0) and extra == 0.0
    held("fitc_lml", body, g0, tag + "fitc lml_grad")
    held("fitc_inducing", gs1[:, :d], gs0, tag + "fitc lml_grad, inducing points")
    assert np.all(gs1[:, d] == 0.0)


# ---- class API -----------------------------------------------------------------------------------------------------------------------
def test_class_api_returns_every_length_key_at_d_17():
    """GP.loglikeParams(returnDeriv=1) on a dense, a FITC and a VFE model (inducingDeriv=True on the sparse ones), looLogLike and
    costFuncEI.derivativeBatch at d = 17, squared exponential: keys cl0 .. cl16, signalSize, noise[, fitcnodes] in that order, and
    out['cl%d' % k] is component k of the reference -- 'noise' times 2 * noise from loglikeParams (gp.py:463-464), the plain
    derivative from looLogLike."""
    from gpExp.gp import GP
    from gpExp.kernels import KernelSquaredExponential
    from gpExp.experimentalDesign import costFuncEI
    kind, d = "se", 17
    c = gc.case(kind, d)
    X, y, S, C = np.array(c.X), np.array(c.y), np.array(c.S), np.array(c.C)
    keys = ["cl%d" % k for k in range(d)] + ["signalSize", "noise"]

    def make(**kw):
        gp = GP(KernelSquaredExponential(list(c.spec["cl"]), c.spec["signalSize"], d), c.noise, **kw)
        if kw:
            gp.fitcnodes = S.copy()
        return gp

    def vector(out, scaled):
        """the dict's entries as the references order them, 'noise' back to the derivative w.r.t. the noise variance"""
        g = np.array([out[k] for k in keys])
        if scaled:
            g[-1] /= 2.0 * c.noise
        return g

    class Space(object):
        dimension = d

    value, out = make().loglikeParams(X, y, returnDeriv=1)
    assert list(out.keys()) == keys and abs(value - gc.reference(kind, d, "lml")[0]) <= 1e-10 * abs(value)
    held("lml", vector(out, True), gc.reference(kind, d, "lml")[1], "loglikeParams, dense")
    value, out = make().looLogLike(X, y, returnDeriv=1)
    assert list(out.keys()) == keys and abs(value - gc.reference(kind, d, "loo")[2]) <= 1e-9 * abs(value)
    held("loo", vector(out, False), gc.reference(kind, d, "loo")[3], "looLogLike")
    for sparse, what, ind in ((None, "fitc_lml", "fitc_inducing"), ("vfe", "vfe", "vfe_inducing")):
        gp = make(FITC=0.5, **({"sparse": sparse} if sparse else {}))
        value, out = gp.loglikeParams(X, y, returnDeriv=1, inducingDeriv=True)
        ref = gc.reference(kind, d, what)
        assert list(out.keys()) == keys + ["fitcnodes"] and np.array_equal(gp.fitcnodes, S)
        assert abs(value - ref[0]) <= 1e-10 * abs(ref[0])
        held(what, vector(out, True), ref[1], "loglikeParams, " + what)
        held(ind, out["fitcnodes"], gc.reference(kind, d, "fitc_inducing") if sparse is None else ref[2], "loglikeParams, " + ind)
        assert list(gp.loglikeParams(X, y, returnDeriv=1)[1].keys()) == keys
    for what, kw in (("acq", {}), ("vfe_acq", dict(FITC=0.5, sparse="vfe"))):
        G = costFuncEI(make(**kw), X, y, 2, Space()).derivativeBatch(C)
        assert G.shape == (gc.M, d)
        held(what, G, gc.reference(kind, d, what)["ei"], "costFuncEI.derivativeBatch, " + what)
