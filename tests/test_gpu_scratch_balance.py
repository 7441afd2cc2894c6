"""The pooled scratch of every entry point goes back to the pool under the size it was taken with (-m gpu).

The pool is keyed by size: gpx_dev_release files a block under the byte count it is TOLD, and a wrong count hands the block out
later as larger than it is.  gpx_dbg_pool_stats keeps the books in pool keys, so a call whose releases match its allocations --
with whatever it returned freed again -- leaves `outstanding_bytes` exactly where it found it.  That is a condition, not a
measurement: the comparison is exact.  Every entry runs twice; the second time every block comes from the pool.

Shapes (d = 3): the smallest that reach each allocation branch --
    N = 300,  M = 260   in-place solve, ragged against the 128-tile, three arg-min partials of 128 candidates
    N = 2100            the out-of-place solve of gpx_posterior / gpx_acq (padded order >= 2048)
    N = 4100, M = 260   the block-inverse scratch of gpx_acq_grad's backward solve (padded order >= 4096)
The factor's explicit block inverses are a cache inside the factor, built by the first solve against it: the model fixture's
gpx_potrs builds them, so that the entries under test start from the steady state."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D, M, NOISE = 3, 260, 1e-2
_models = {}


def model(n):
    """(ctx, spec, X, L, y, alpha, Z, host X) for n training points; built once per size and left unchanged."""
    from gpexp_amd import device as dev
    if n not in _models:
        ctx = dev.context()
        rng = np.random.RandomState(1000 + n)
        Xh = rng.uniform(-1.0, 1.0, (n, D))
        Zh = rng.uniform(-1.0, 1.0, (M, D))
        y = np.sin(3.0 * Xh[:, 0]) + Xh[:, 1] * Xh[:, 2]
        spec = dev.KernelSpec(dev.K_SE, D, [0.5, 0.7, 0.6, 1.3])
        X, Z = dev.points(ctx, Xh), dev.points(ctx, Zh)
        L = dev.potrf(ctx, dev.kfill(ctx, spec, X, nugget=NOISE))
        alpha = dev.potrs(ctx, L, y)
        _models[n] = (ctx, spec, X, L, y, alpha, Z, Xh)
    return _models[n]


def release(ctx, obj):
    from gpexp_amd import device as dev
    if isinstance(obj, dev.DeviceMatrix):
        obj.free()
    elif isinstance(obj, dev.FitcModel):
        ctx.lib.gpx_fitc_free(ctx.h, obj.h)
        obj.h = None
    elif isinstance(obj, (tuple, list)):
        for o in obj:
            release(ctx, o)


def balanced(ctx, call):
    for rep in range(2):
        before = ctx.pool_stats()[1]
        release(ctx, call())
        after = ctx.pool_stats()[1]
        print("call %d: outstanding %d -> %d bytes" % (rep, before, after))
        assert after == before, "call %d left %d bytes of pool keys outstanding" % (rep, after - before)


def _posterior(n):
    from gpexp_amd import device as dev
    ctx, spec, X, L, y, alpha, Z, Xh = model(n)
    return ctx, lambda: dev.posterior(ctx, spec, L, X, alpha, Z)


def _ivar(n):
    from gpexp_amd import device as dev
    ctx, spec, X, L, y, alpha, Z, Xh = model(n)
    return ctx, lambda: dev.ivar(ctx, spec, L, X, Z)


def _ivar_keep_update(n):
    from gpexp_amd import device as dev
    ctx, spec, X, L, y, alpha, Z, Xh = model(n)

    def call():
        cost, W = dev.ivar(ctx, spec, L, X, Z, keep=True)
        assert W is not None
        dev.ivar_update(ctx, spec, L, X, Z, W, 128)
        return W
    return ctx, call


def _potrs(n):
    from gpexp_amd import device as dev
    ctx, spec, X, L, y, alpha, Z, Xh = model(n)
    return ctx, lambda: dev.potrs(ctx, L, y)


def _kdiag(n):
    from gpexp_amd import device as dev
    ctx, spec, X, L, y, alpha, Z, Xh = model(n)
    return ctx, lambda: dev.kdiag(ctx, spec, Z)


def _acq(n):
    from gpexp_amd import device as dev
    ctx, spec, X, L, y, alpha, Z, Xh = model(n)
    return ctx, lambda: dev.acq(ctx, spec, L, X, alpha, Z, dev.ACQ_EI, float(y.max()))


def _acq_grad(n):
    from gpexp_amd import device as dev
    ctx, spec, X, L, y, alpha, Z, Xh = model(n)
    return ctx, lambda: dev.acq_grad(ctx, spec, L, X, alpha, Z, dev.ACQ_EI, float(y.max()))


def _acq_batch(n):
    from gpexp_amd import device as dev
    ctx, spec, X, L, y, alpha, Z, Xh = model(n)
    return ctx, lambda: dev.acq_batch(ctx, spec, L, X, alpha, Z, NOISE, dev.ACQ_EI, float(y.max()), True, dev.LIE_BELIEVER,
                                      0.0, 3, want_all=True)


def _ivar_grad(n):
    from gpexp_amd import device as dev
    ctx, spec, X, L, y, alpha, Z, Xh = model(n)
    return ctx, lambda: dev.ivar_grad(ctx, spec, L, X, Z)


def _var_grad_newpt(n):
    from gpexp_amd import device as dev
    ctx, spec, X, L, y, alpha, Z, Xh = model(n)
    return ctx, lambda: dev.var_grad_newpt(ctx, spec, L, X, Z)


def _lml_grad(n):
    from gpexp_amd import device as dev
    ctx, spec, X, L, y, alpha, Z, Xh = model(n)
    return ctx, lambda: dev.lml_grad_full(ctx, spec, L, X, alpha)


def _mi_greedy(n):
    from gpexp_amd import device as dev
    ctx, spec, X, L, y, alpha, Z, Xh = model(n)
    return ctx, lambda: dev.mi_greedy(ctx, spec, Z, NOISE, 4)


def _greedy_var(n):
    from gpexp_amd import device as dev
    ctx, spec, X, L, y, alpha, Z, Xh = model(n)
    return ctx, lambda: dev.greedy_var(ctx, spec, Z, 4)


def _loo(n):
    from gpexp_amd import device as dev
    ctx, spec, X, L, y, alpha, Z, Xh = model(n)
    return ctx, lambda: dev.loo(ctx, L, y)


def _loo_grad(n):
    from gpexp_amd import device as dev
    ctx, spec, X, L, y, alpha, Z, Xh = model(n)
    return ctx, lambda: dev.loo_grad(ctx, spec, L, X, NOISE, y)


def _fitc(n):
    from gpexp_amd import device as dev
    ctx, spec, X, L, y, alpha, Z, Xh = model(n)

    def call():
        S = dev.points(ctx, Xh[:40])
        f = dev.FitcModel(ctx, spec, X, S, NOISE)
        f.solve(y)
        return f, S
    return ctx, call


ENTRIES = [
    ("posterior", _posterior, 300), ("posterior", _posterior, 2100),
    ("ivar", _ivar, 300), ("ivar_keep+ivar_update", _ivar_keep_update, 300),
    ("potrs", _potrs, 300), ("kdiag", _kdiag, 300),
    ("acq", _acq, 300), ("acq", _acq, 2100),
    ("acq_grad", _acq_grad, 300), ("acq_grad", _acq_grad, 4100),
    ("acq_batch", _acq_batch, 300),
    ("ivar_grad", _ivar_grad, 300), ("var_grad_newpt", _var_grad_newpt, 300),
    ("lml_grad", _lml_grad, 300), ("mi_greedy", _mi_greedy, 300), ("greedy_var", _greedy_var, 300),
    ("loo", _loo, 300), ("loo_grad", _loo_grad, 300),
    ("fitc_fit+fitc_solve", _fitc, 300),
]


@pytest.mark.parametrize("name,make,n", ENTRIES, ids=["%s-N%d" % (e[0], e[2]) for e in ENTRIES])
def test_outstanding_bytes_return_to_their_value(name, make, n):
    ctx, call = make(n)
    balanced(ctx, call)
