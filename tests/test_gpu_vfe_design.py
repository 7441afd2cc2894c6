"""IVAR design on a VFE model on the device (gpx_vfe_design_*, gpx_vfe_var_grad*, device.VfeDesign, GP.vfeVarianceGradient*,
costFunctionVFE_IVAR) against the NumPy forms of tests/vfe_design_ref.py, which tests/test_vfe_design_host.py ties to each other
and to central differences.

Tolerances are the project's own figures: the cost within 1e-8 signalSize of the direct per-point form (tests/test_gpu_vfe.py's
predictor figure) and of the path that existed before (gpx_vfe_posterior + a host mean); the gradient and both point-wise
derivatives within 1e-8 of the largest |entry| of the closed forms (the figure of gpx_vfe_acq_grad and dF/dS); the directional
central difference of the DEVICE cost within 1e-6 of sum |grad|.  Every input has min var >= 0.028 signalSize: nothing sits on a
cancellation.

Shapes: the six cases of fitc_grad_ref (nu = 129 / N = 257 one past a 128 tile, nu = 40 below one tile, nu = 257), BLOCKED
(nu = 1152: chol(A) and the two-sided solve cross the 1024-order block inverses), an out-of-place case (nu = 2049: the left solve
through the block inverses), M = 300 with five training points among them and M = 1, pinned counts 0, 1, 128 and N - 1 (b = 1), and
the dimension sweep of grad_dims_cases (d = 2, 9, 16, 17, 32 times three kernels)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import fitc_grad_ref as ref
import grad_dims_cases as gd
import vfe_design_ref as dref

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
CASES = dict(zip(ref.IDS, ref.CASES))
LARGE = {"blocked-m52-d8-nu1152": ref.BLOCKED, "oop-m52-d8-nu2049": ("matern52", 8, [1.5], 1.2, 2304, 2049, 0.05, 19)}
CASES.update(LARGE)
PINNED_LARGE = 2048


@functools.lru_cache(maxsize=None)
def problem(cid):
    """(spec, X, S, noise, Z): drawn once, shared, read-only."""
    if cid in CASES:
        spec, X, S, _, noise = ref.case(CASES[cid])
        Z = np.random.default_rng(31).uniform(-1.2, 1.2, (300, spec["d"]))
        Z[:5] = X[:5]
    else:
        c = gd.case(*gd.PARAMS[gd.IDS.index(cid)])
        spec, X, S, noise, Z = c.spec, c.X, c.S, c.noise, c.Z
    for a in (X, S, Z):
        a.setflags(write=False)
    return spec, X, S, noise, Z


@functools.lru_cache(maxsize=None)
def reference(cid, m1=False):
    """(cost, gradient (N, d)) of the closed forms, once per case."""
    spec, X, S, noise, Z = problem(cid)
    Z = Z[7:8] if m1 else Z
    G = dref.grad(spec, X, S, noise, Z)
    G.setflags(write=False)
    return dref.cost(spec, X, S, noise, Z), G


@functools.lru_cache(maxsize=None)
def point_references(cid):
    spec, X, S, noise, Z = problem(cid)
    out = dref.var_grad(spec, X, S, noise, Z), dref.var_grad_newpt(spec, X, S, noise, Z)
    for a in out:
        a.setflags(write=False)
    return out


def kernel_spec(spec):
    from gpexp_amd import device as dev
    return dev.KernelSpec(ref.KIND_ID[spec["kind"]], spec["d"], ref.hyp_of(spec))


def design(cid, Z=None):
    from gpexp_amd import device as dev
    spec, X, S, noise, Z0 = problem(cid)
    ctx = dev.context()
    return dev, ctx, dev.VfeDesign(ctx, kernel_spec(spec), dev.points(ctx, S), noise, dev.points(ctx, Z0 if Z is None else Z))


def split_eval(dev, ctx, ds, X, r0, want_grad=True):
    ds.pin(dev.points(ctx, X[:r0]) if r0 > 0 else None)
    return ds.eval(dev.points(ctx, X[r0:]), want_grad=want_grad)


def model(cid):
    from gpexp_amd import device as dev
    spec, X, S, noise, Z = problem(cid)
    ctx = dev.context()
    ks = kernel_spec(spec)
    return dev, ctx, ks, dev.VfeModel(ctx, ks, dev.points(ctx, X), dev.points(ctx, S), noise)


def make_gp(spec, noise, **kw):
    from gpExp.kernels import KernelIsoMatern, KernelSquaredExponential
    from gpExp.gp import GP
    if spec["kind"] == "se":
        k = KernelSquaredExponential(list(spec["cl"]), spec["signalSize"], spec["d"])
    else:
        k = KernelIsoMatern(spec["rho"], spec["signalSize"], spec["d"], nu=1.5 if spec["kind"] == "matern32" else 2.5)
    return GP(k, noise, **kw)


def max_relerr(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


# ---- 1. cost and gradient ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ref.IDS)
def test_cost_and_gradient_match_the_closed_forms(cid):
    """Pinned counts 0, 1, 128 and N - 1; each split also against the same design all free (not bit for bit: A is summed in
    another order).  Measured worst over the six cases: cost 4.0e-15, gradient 3.8e-12, split against all free 5.0e-15 / 3.9e-12."""
    spec, X, S, noise, Z = problem(cid)
    c_ref, G = reference(cid)
    s, n = spec["signalSize"], X.shape[0]
    dev, ctx, ds = design(cid)
    assert ds.shape() == (S.shape[0], Z.shape[0], 0)
    c0, g0 = split_eval(dev, ctx, ds, X, 0)
    worst = dict(cost=0.0, grad=0.0, split_cost=0.0, split_grad=0.0)
    for r0 in (0, 1, 128, n - 1):
        c, g = split_eval(dev, ctx, ds, X, r0)
        assert ds.shape()[2] == r0 and g.shape == (n - r0, X.shape[1])
        worst["cost"] = max(worst["cost"], abs(c - c_ref) / s)
        worst["grad"] = max(worst["grad"], max_relerr(g, G[r0:]))
        worst["split_cost"] = max(worst["split_cost"], abs(c - c0) / s)
        worst["split_grad"] = max(worst["split_grad"], max_relerr(g, g0[r0:]))
        assert split_eval(dev, ctx, ds, X, r0, want_grad=False) == (c, None)     # the cost alone: the same bits
    print(cid, " ".join("%s %.2e" % kv for kv in worst.items()))
    assert worst["cost"] <= 1e-8 and worst["split_cost"] <= 1e-8, worst
    assert worst["grad"] <= 1e-8 and worst["split_grad"] <= 1e-8, worst


@pytest.mark.parametrize("cid", list(LARGE))
def test_large_orders_with_pinned_points(cid):
    """nu = 1152 and nu = 2049 with 2048 of the 2304 points pinned: the reference's gradient restricted to the free rows.
    Measured: cost 1.3e-14 / 6.4e-14, gradient 1.4e-10 / 1.4e-10."""
    spec, X, S, noise, Z = problem(cid)
    c_ref, G = reference(cid)
    dev, ctx, ds = design(cid)
    c, g = split_eval(dev, ctx, ds, X, PINNED_LARGE)
    errs = dict(cost=abs(c - c_ref) / spec["signalSize"], grad=max_relerr(g, G[PINNED_LARGE:]))
    print(cid, " ".join("%s %.2e" % kv for kv in errs.items()))
    assert errs["cost"] <= 1e-8 and errs["grad"] <= 1e-8, errs


def test_one_monte_carlo_point():
    cid = "m52-d8"
    spec, X, S, noise, Z = problem(cid)
    c_ref, G = reference(cid, True)
    dev, ctx, ds = design(cid, Z[7:8])
    c, g = split_eval(dev, ctx, ds, X, 0)
    errs = dict(cost=abs(c - c_ref) / spec["signalSize"], grad=max_relerr(g, G))
    print(cid, "M = 1:", " ".join("%s %.2e" % kv for kv in errs.items()))
    assert errs["cost"] <= 1e-8 and errs["grad"] <= 1e-8, errs


@pytest.mark.parametrize("cid", ["se-d3", "m52-d8"])
def test_gradient_against_a_directional_difference_of_the_device_cost(cid):
    """Along sign(grad), h = 1e-5: within 1e-6 of sum |grad|.  Measured 8.3e-10 (se-d3), 3.8e-9 (m52-d8)."""
    spec, X, S, noise, Z = problem(cid)
    dev, ctx, ds = design(cid)
    c, g = split_eval(dev, ctx, ds, X, 0)
    V = np.sign(g)
    fd = dref.directional_fd(lambda P: ds.eval(dev.points(ctx, P), want_grad=False)[0], np.array(X), V, 1e-5)
    err = abs(fd - float(np.sum(g * V))) / float(np.sum(np.abs(g)))
    print("%s: directional difference of the device cost %.2e" % (cid, err))
    assert err <= 1e-6, err


# ---- 2. the point-wise derivatives ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ref.IDS)
def test_point_wise_derivatives_match_the_closed_forms(cid):
    """Measured worst over the six cases: full 3.6e-12, newpt 3.1e-13."""
    spec, X, S, noise, Z = problem(cid)
    full_ref, newpt_ref = point_references(cid)
    dev, ctx, ks, m = model(cid)
    Zd = dev.points(ctx, Z)
    full = m.design_var_grad(ks, m.X, m.S, Zd)
    newpt = m.design_var_grad_newpt(m.S, Zd)
    errs = dict(full=max_relerr(full, full_ref), newpt=max_relerr(newpt, newpt_ref))
    print(cid, " ".join("%s %.2e" % kv for kv in errs.items()))
    assert full.shape == full_ref.shape and newpt.shape == newpt_ref.shape
    assert errs["full"] <= 1e-8 and errs["newpt"] <= 1e-8, errs
    # M = 1
    one = m.design_var_grad(ks, m.X, m.S, dev.points(ctx, Z[7:8]))
    assert max_relerr(one[:, 0], full_ref[:, 7]) <= 1e-8


@pytest.mark.parametrize("cid", gd.IDS)
def test_dimension_sweep(cid):
    """d = 2, 9, 16, 17, 32 times three kernels, N = 300, nu = M = 70: gpx_vfe_design_eval, gpx_vfe_var_grad, gpx_vfe_var_grad_newpt.
    Measured worst over the 15 cases: cost 4.1e-14, gradient 1.2e-10, full 8.9e-11, newpt 1.1e-11."""
    spec, X, S, noise, Z = problem(cid)
    c_ref, G = reference(cid)
    full_ref, newpt_ref = point_references(cid)
    dev, ctx, ds = design(cid)
    c, g = split_eval(dev, ctx, ds, X, 0)
    c2, g2 = split_eval(dev, ctx, ds, X, 128)
    _, _, ks, m = model(cid)
    Zd = dev.points(ctx, Z)
    errs = dict(cost=max(abs(c - c_ref), abs(c2 - c_ref)) / spec["signalSize"], grad=max(max_relerr(g, G), max_relerr(g2, G[128:])),
                full=max_relerr(m.design_var_grad(ks, m.X, m.S, Zd), full_ref),
                newpt=max_relerr(m.design_var_grad_newpt(m.S, Zd), newpt_ref))
    print(cid, " ".join("%s %.2e" % kv for kv in errs.items()))
    assert errs["cost"] <= 1e-8 and max(errs["grad"], errs["full"], errs["newpt"]) <= 1e-8, errs


# ---- 3. contracts ------------------------------------------------------------------------------------------------------------------
def digest(cids=("se-d8", "m32-d8-nu257")):
    out = []
    for cid in cids:
        spec, X, S, noise, Z = problem(cid)
        dev, ctx, ds = design(cid)
        c, g = split_eval(dev, ctx, ds, X, 128)
        _, _, ks, m = model(cid)
        Zd = dev.points(ctx, Z[:40])
        out.append(np.concatenate([[c], g.ravel(), m.design_var_grad(ks, m.X, m.S, Zd).ravel(),
                                   m.design_var_grad_newpt(m.S, Zd)]).tobytes().hex())
    ctx.sync()
    return "%s %d" % ("".join(out), int(ctx.lib.gpx_dbg_guard_violations(ctx.h)))


def test_two_calls_agree_bit_for_bit():
    assert digest().split()[0] == digest().split()[0]


def child(call, **env):
    code = "import sys\nsys.path[:0] = [%r, %r]\nimport test_gpu_vfe_design as t\nprint('RESULT ' + t.%s, flush=True)" % (ROOT, TESTS, call)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    return [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][0][7:]


def test_same_bits_under_chaos_and_nan_filled_guarded_blocks():
    """One child process with GPX_CHAOS (launch sites held back at random) and GPX_ALLOC_GUARD=2 (guard bands; blocks handed out
    NaN-filled): the same bits, no violation."""
    here = digest().split()[0]
    bits, violations = child("digest()", GPX_CHAOS="7", GPX_ALLOC_GUARD="2").split()
    assert violations == "0"
    assert bits == here


def chunked_values(cid="m32-d8-nu257"):
    spec, X, S, noise, Z = problem(cid)
    dev, ctx, ds = design(cid)
    c, g = split_eval(dev, ctx, ds, X, 0)
    return np.concatenate([[c], g.ravel()]).tobytes().hex()


def test_gram_matrix_accumulated_over_three_chunks():
    """A child whose GPX_CROSS_BYTES allows 128 MC points per chunk (nu = 257 pads to 384 rows): M = 300 runs as chunks of 128, 128
    and 44.  Another summation order of Gz: within the tolerances, not the same bits.  Measured: cost 1.4e-16, gradient 1.3e-12;
    largest difference from the one-chunk run 5.0e-16."""
    cid = "m32-d8-nu257"
    spec = problem(cid)[0]
    c_ref, G = reference(cid)
    v = np.frombuffer(bytes.fromhex(child("chunked_values()", GPX_CROSS_BYTES=str(384 * 8 * 128))), dtype=np.float64)
    here = np.frombuffer(bytes.fromhex(chunked_values()), dtype=np.float64)
    errs = dict(cost=abs(v[0] - c_ref) / spec["signalSize"], grad=max_relerr(v[1:], G.ravel()),
                against_one_chunk=float(np.max(np.abs(v - here))))
    print(cid, " ".join("%s %.2e" % kv for kv in errs.items()))
    assert errs["cost"] <= 1e-8 and errs["grad"] <= 1e-8, errs


def test_pooled_bytes_return_after_create_eval_free():
    cid = "m52-d8"
    spec, X, S, noise, Z = problem(cid)
    from gpexp_amd import device as dev
    ctx = dev.context()
    Xd = dev.points(ctx, X)
    for _ in range(2):
        ctx.sync()
        before = ctx.pool_stats()[1]
        _, _, ds = design(cid)
        ds.pin(dev.points(ctx, X[:100]))
        mid = ctx.pool_stats()[1]
        ds.eval(Xd)
        assert ctx.pool_stats()[1] == mid          # eval and pin leave nothing out
        del ds
        ctx.sync()
        assert ctx.pool_stats()[1] == before


def test_mehler_has_a_cost_and_no_gradient():
    from gpExp.kernels import KernelMehlerND
    from gpexp_amd import device as dev
    rng = np.random.default_rng(3)
    X, Z = rng.uniform(-1.0, 1.0, (150, 2)), rng.uniform(-1.0, 1.0, (200, 2))
    ctx = dev.context()
    ks = KernelMehlerND([0.5, 0.3], 2)._spec()
    S = dev.points(ctx, X[:60])
    ds = dev.VfeDesign(ctx, ks, S, 0.05, dev.points(ctx, Z))
    c, g = ds.eval(dev.points(ctx, X), want_grad=False)
    m = dev.VfeModel(ctx, ks, dev.points(ctx, X), S, 0.05)
    var = m.posterior(None, dev.points(ctx, Z), want_mean=False)[1]
    assert g is None and abs(c - np.mean(var)) <= 1e-8 * np.max(np.abs(var))
    with pytest.raises(dev.GpxError, match="Mehler"):
        ds.eval(dev.points(ctx, X))
    with pytest.raises(dev.GpxError, match="Mehler"):
        m.design_var_grad_newpt(S, dev.points(ctx, Z))


def test_refusals():
    dev, ctx, ks, vfe = model("se-d3")
    spec, X, S, noise, Z = problem("se-d3")
    fitc = dev.FitcModel(ctx, ks, dev.points(ctx, X), dev.points(ctx, S), noise)
    Zd = dev.points(ctx, Z[:7])
    with pytest.raises(dev.GpxError, match=r"gpx_fitc_var_grad\b"):
        dev.VfeModel.design_var_grad(fitc, ks, fitc.X, fitc.S, Zd)
    with pytest.raises(dev.GpxError, match="gpx_fitc_var_grad_newpt"):
        dev.VfeModel.design_var_grad_newpt(fitc, fitc.S, Zd)
    other = dev.KernelSpec(ks.kind, ks.d, ks.hyp * 1.1)
    with pytest.raises(dev.GpxError, match="not the kernel"):
        vfe.design_var_grad(other, vfe.X, vfe.S, Zd)
    _, _, ds = design("se-d3")
    with pytest.raises(dev.GpxError, match="at least one free"):
        ds.eval(dev.points(ctx, np.zeros((0, spec["d"]))))
    for bad in (0.0, -0.1):
        with pytest.raises(dev.GpxError, match="noise"):
            dev.VfeDesign(ctx, ks, dev.points(ctx, S), bad, Zd)
    # the refusals that stay: the existing point-derivative entries on a VFE handle
    with pytest.raises(dev.GpxError, match="gpx_vfe_posterior"):
        vfe.var_grad(ks, Zd)


# ---- 4. class API ------------------------------------------------------------------------------------------------------------------
def design_gp(cid):
    from gpExp.approximation import Space
    spec, X, S, noise, Z = problem(cid)
    rng = np.random.default_rng(2)
    space = Space(spec["d"], lambda size: rng.uniform(-1, 1, size), lambda p: np.ones(len(p)))
    gp = make_gp(spec, noise, FITC=0.5, sparse="vfe")
    gp.fitcnodes = np.array(S)
    return spec, np.array(X), noise, np.array(Z), space, gp


@pytest.mark.parametrize("cid", ["se-d3", "m52-d8"])
def test_class_api(cid):
    """se-d3 runs with signalSize = 1.7: the squared exponential's TRUE derivative (no doubled signalSize) is what is compared.
    Measured: cost 2.1e-15, against the earlier path 1.1e-15, gradients <= 3.7e-12, column mean of vfeVarianceGradient against
    costFunctionVFE_IVAR.derivative <= 4.5e-12."""
    from gpExp.experimentalDesign import costFunctionGP_IVAR, costFunctionVFE_IVAR
    spec, X, noise, Z, space, gp = design_gp(cid)
    c_ref, G = reference(cid)
    s, n, d = spec["signalSize"], X.shape[0], spec["d"]
    cf = costFunctionVFE_IVAR(gp, n, space, mcPoints=Z)
    cost, g = cf.evaluate(X), cf.derivative(X)
    old = costFunctionGP_IVAR(gp, n, space, mcPoints=Z).evaluate(X)           # gpx_vfe_posterior, then a host mean
    c2, g2 = cf.evaluateWithDerivative(X)
    assert isinstance(cost, float) and g.shape == (n * d,) and g.dtype == np.float64 and c2 == cost and np.array_equal(g2, g)
    cf.pinnedPoints = 128
    gp_ = cf.derivative(X)
    assert np.all(gp_[:128 * d] == 0.0)
    # the literal matrix of the model fitted at X: its column mean is the same gradient
    gp.addNodesAndComputeCovariance(X)
    full = gp.vfeVarianceGradient(Z)
    newpt = gp.vfeVarianceGradientWRTnewpt(Z)
    full_ref, newpt_ref = point_references(cid)
    errs = dict(cost=abs(cost - abs(c_ref)) / s, old_path=abs(cost - old) / s, grad=max_relerr(g, G.ravel()),
                pinned=max_relerr(gp_[128 * d:], G[128:].ravel()), full=max_relerr(full, full_ref), newpt=max_relerr(newpt, newpt_ref),
                mean_of_full_against_derivative=max_relerr(full.mean(axis=1), g))
    print(cid, " ".join("%s %.2e" % kv for kv in errs.items()))
    assert full.shape == (n * d, len(Z)) and newpt.shape == (len(Z) * d,)
    assert errs["cost"] <= 1e-8 and errs["old_path"] <= 1e-8, errs
    assert max(errs["grad"], errs["pinned"], errs["full"], errs["newpt"]) <= 1e-8, errs
    # refusals of the new names
    for other in (make_gp(spec, noise), make_gp(spec, noise, FITC=0.5)):
        other.addNodesAndComputeCovariance(X)
        with pytest.raises(ValueError, match="VFE"):
            other.vfeVarianceGradient(Z)
        with pytest.raises(ValueError, match="VFE"):
            other.vfeVarianceGradientWRTnewpt(Z)
    with pytest.raises(NotImplementedError, match="nodes"):
        make_gp(spec, noise, FITC=0.5, sparse="vfe").vfeVarianceGradient(Z)
    with pytest.raises(NotImplementedError, match="VFE"):                     # the existing name keeps refusing
        gp.varianceGradient(Z)


def test_mehler_class_api():
    from gpExp.kernels import KernelMehlerND
    from gpExp.gp import GP
    from gpExp.approximation import Space
    from gpExp.experimentalDesign import costFunctionVFE_IVAR
    rng = np.random.default_rng(3)
    X, Z = rng.uniform(-1.0, 1.0, (150, 2)), rng.uniform(-1.0, 1.0, (200, 2))
    gp = GP(KernelMehlerND([0.5, 0.3], 2), 0.05, FITC=0.5, sparse="vfe")
    gp.fitcnodes = X[:60].copy()
    cf = costFunctionVFE_IVAR(gp, len(X), Space(2, lambda size: rng.uniform(-1, 1, size), lambda p: np.ones(len(p))), mcPoints=Z)
    assert np.isfinite(cf.evaluate(X))
    with pytest.raises(NotImplementedError, match="KernelMehlerND"):
        cf.derivative(X)
    gp.addNodesAndComputeCovariance(X)
    with pytest.raises(NotImplementedError, match="KernelMehlerND"):
        gp.vfeVarianceGradient(Z)


def small_design():
    from gpExp.experimentalDesign import costFunctionVFE_IVAR
    spec, X, noise, Z, space, gp = design_gp("se-d3")
    gp.fitcnodes = np.array(X[:40])
    return spec, X, Z[:200], space, gp, costFunctionVFE_IVAR


def test_slsqp_design_does_not_increase_the_cost():
    from gpExp.experimentalDesign import ExperimentalDesignDerivative
    spec, X, Z, space, gp, Cost = small_design()
    d = spec["d"]
    cf = Cost(gp, 12, space, mcPoints=Z)
    X0 = np.array(X[100:112])
    start = cf.evaluate(X0)
    pts = ExperimentalDesignDerivative(cf, 12, d).begin([X0], -1.2 * np.ones(12 * d), 1.2 * np.ones(12 * d))
    end = cf.evaluate(pts)
    print("SLSQP on the VFE cost: %.6f -> %.6f" % (start, end))
    assert pts.shape == (12, d) and end <= start


def test_batch_greedy_design_keeps_the_earlier_batches(monkeypatch):
    from gpExp import experimentalDesign as ed
    spec, X, Z, space, gp, Cost = small_design()
    d = spec["d"]
    batches = []
    inner = ed.ExperimentalDesignDerivative.beginWithVarGreedy

    def recording(self, *a, **kw):
        out = inner(self, *a, **kw)
        batches.append((type(self.costFunction), np.array(out)))
        return out

    monkeypatch.setattr(ed.ExperimentalDesignDerivative, "beginWithVarGreedy", recording)
    pts = ed.ExperimentalDesignGreedyWithDerivatives(Cost(gp, 4, space, mcPoints=Z), 12, 4, d).begin()
    assert pts.shape == (12, d) and [b[0] for b in batches] == [Cost] * 3
    assert [len(b[1]) for b in batches] == [4, 8, 12]
    assert np.array_equal(pts[:8], batches[1][1]) and np.array_equal(pts[:4], batches[0][1])
