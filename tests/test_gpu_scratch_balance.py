"""The pooled scratch of every entry point goes back to the pool under the size it was taken with (-m gpu).

The pool is keyed by size: gpx_dev_release files a block under the byte count it is TOLD, and a wrong count hands the block out
later as larger than it is.  gpx_dbg_pool_stats keeps the books in pool keys, so a call whose releases match its allocations --
with whatever it returned freed again -- leaves `outstanding_bytes` exactly where it found it.  That is a condition, not a
measurement: the comparison is exact.  Every entry runs twice; the second time every block comes from the pool.

Shapes (d = 3): the smallest that reach each allocation branch --
    N = 300,  M = 260   in-place solve, ragged against the 128-tile, three arg-min partials of 128 candidates
    N = 2100            the out-of-place solve of gpx_posterior / gpx_acq / gpx_acq_batch's set-up (padded order >= 2048)
    N = 4100, M = 260   the block-inverse scratch of gpx_acq_grad's backward solve (padded order >= 4096)
    257 / 2049 inducing points (at N = 300 / 2100)   the in-place and the out-of-place set-up of the sparse predictors
The entries whose passes are chunked (CHUNKED) run a second time with GPX_CROSS_BYTES=1: chunks of 128, 128 and 4 points.
The factor's explicit block inverses are a cache inside the factor, built by the first solve against it: the model fixture's
gpx_potrs builds them, so that the entries under test start from the steady state.

FAILURE EXITS.  The same books must balance when an entry gives up half way.  Every case below is a call that answers with a
non-zero status AFTER it has taken pooled memory: a nugget / noise of -2 on a kernel of signal variance 1.3 makes the first pivot
the factorisation meets negative, which it REPORTS (a status, nothing is provoked on the device).  Asserted per case: GpxError,
`outstanding_bytes` exactly where it was, and the same entry called validly right afterwards returns, byte for byte, what it
returns in a process that never saw the failure (one child process computes those digests for all cases).
    refit_rows  N = 300, keep = 128     the in-place strip solve, main stream only
    refit_rows  N = 4500, keep = 4096   the copy of the kept rows on the side stream + the `wide` scratch scope (one more model)
    mi_greedy, mi_begin                 260 candidates: gpx_potrf of K(C, C) - 2 I fails inside the call, S is handed back
    fitc_fit    N = 300, 64 inducing    the first in-place factorisation fails with the model half built
None of them is rejected by an argument check before the first allocation."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

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


def _dbg_greedy_var_scores(n):
    from gpexp_amd import device as dev
    ctx, spec, X, L, y, alpha, Z, Xh = model(n)
    return ctx, lambda: dev.dbg_greedy_var_scores(ctx, spec, Z, keep=[5, 200, 17])


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


def _var_grad(n):
    from gpexp_amd import device as dev
    ctx, spec, X, L, y, alpha, Z, Xh = model(n)
    return ctx, lambda: dev.var_grad(ctx, spec, L, X, Z)


def _posterior_cov(n):
    from gpexp_amd import device as dev
    ctx, spec, X, L, y, alpha, Z, Xh = model(n)
    return ctx, lambda: dev.posterior_cov(ctx, spec, L, X, Z)


def _greedy_ivar_step(n):
    from gpexp_amd import device as dev
    ctx, spec, X, L, y, alpha, Z, Xh = model(n)
    Zmc = dev.points(ctx, np.random.RandomState(7).uniform(-1.0, 1.0, (150, D)))
    return ctx, lambda: dev.greedy_ivar_step(ctx, spec, L, X, Z, Zmc, NOISE)


def _psampler(n, prior=False):
    from gpexp_amd import device as dev
    ctx, spec, X, L, y, alpha, Z, Xh = model(n)
    xi = np.random.RandomState(11).standard_normal((5, M))

    def call():
        ps = dev.PosteriorSampler(ctx, spec, *((None, None, None) if prior else (L, X, alpha)), Z, 1e-6)
        out = (ps.draw(xi),) + ps.argbest(xi) + ps.argbest(xi, minimize=False)
        ps.close()
        return out
    return ctx, call


def _psampler_prior(n):
    return _psampler(n, prior=True)


def _acq_qei(n):
    from gpexp_amd import device as dev
    ctx, spec, X, L, y, alpha, Z, Xh = model(n)
    rng = np.random.RandomState(13)
    Zb, xi = dev.points(ctx, rng.uniform(-1.0, 1.0, (5 * 3, D))), rng.standard_normal((8, 3))
    return ctx, lambda: dev.acq_qei(ctx, spec, L, X, alpha, Zb, 3, xi, float(y.min()), 1e-8)


def _paths(n):
    from gpexp_amd import device as dev
    ctx, spec, X, L, y, alpha, Z, Xh = model(n)
    rng = np.random.RandomState(17)
    omega, phase = rng.standard_normal((40, D)) / np.array([0.5, 0.7, 0.6]), rng.uniform(0.0, 2.0 * np.pi, 40)
    w, eps = rng.standard_normal((3, 40)), np.sqrt(NOISE) * rng.standard_normal((3, n))
    Zp = dev.points(ctx, rng.uniform(-1.0, 1.0, (4, D)))

    def call():
        ps = dev.PathSampler(ctx, spec, L, X, alpha, omega, phase, w, eps)
        out = ps.argbest(Z, want_values=True) + ps.argbest(Z, minimize=False) + ps.gradient(Zp, [0, 2, 1, 0], want_values=True)
        ps.close()
        return out
    return ctx, call


_sparse = {}


def sparse_model(n, nu, vfe):
    """(model, coeff) on the first nu training points as inducing points; built once per shape and left unchanged."""
    from gpexp_amd import device as dev
    if (n, nu, vfe) not in _sparse:
        ctx, spec, X, L, y, alpha, Z, Xh = model(n)
        f = (dev.VfeModel if vfe else dev.FitcModel)(ctx, spec, X, dev.points(ctx, Xh[:nu]), NOISE)
        _sparse[(n, nu, vfe)] = (f, f.solve(y)[0])
    return _sparse[(n, nu, vfe)]


def _fitc_posterior(n):
    ctx, (f, coeff), Z = model(n)[0], sparse_model(n, 257, False), model(n)[6]
    return ctx, lambda: f.posterior(coeff, Z)


def _vfe(what, nu):
    def make(n):
        from gpexp_amd import device as dev
        ctx, (f, coeff), y, Z = model(n)[0], sparse_model(n, nu, True), model(n)[4], model(n)[6]
        return ctx, {
            "posterior": lambda: f.posterior(coeff, Z),
            "acq": lambda: f.acq(coeff, Z, dev.ACQ_EI, float(y.max())),
            "acq_grad": lambda: f.acq_grad(coeff, Z, dev.ACQ_EI, float(y.max())),
            "acq_batch": lambda: f.acq_batch(coeff, Z, dev.ACQ_EI, float(y.max()), True, dev.LIE_BELIEVER, 0.0, 3, want_all=True),
        }[what]
    return make


VFE_CALLS = ("posterior", "acq", "acq_grad", "acq_batch")
# the entries whose passes are chunked under GPX_CROSS_BYTES: run at the default budget (with ENTRIES) and at a budget of one
# byte, where every rule clamps to chunks of 128 -- M = 260 in three chunks, the last of 4 points
CHUNKED = [
    ("posterior_cov", _posterior_cov, 300), ("greedy_ivar_step", _greedy_ivar_step, 300),
    ("psampler", _psampler, 300), ("psampler_prior", _psampler_prior, 300),
    ("acq_qei", _acq_qei, 300), ("acq_qei", _acq_qei, 2100),
    ("paths", _paths, 300), ("fitc_posterior", _fitc_posterior, 300), ("var_grad", _var_grad, 300),
] + [("vfe_%s" % c, _vfe(c, 257), 300) for c in VFE_CALLS] + [("vfe_%s_nu2049" % c, _vfe(c, 2049), 2100) for c in VFE_CALLS]

ENTRIES = [
    ("posterior", _posterior, 300), ("posterior", _posterior, 2100),
    ("ivar", _ivar, 300), ("ivar_keep+ivar_update", _ivar_keep_update, 300),
    ("potrs", _potrs, 300), ("kdiag", _kdiag, 300),
    ("acq", _acq, 300), ("acq", _acq, 2100),
    ("acq_grad", _acq_grad, 300), ("acq_grad", _acq_grad, 4100),
    ("acq_batch", _acq_batch, 300), ("acq_batch", _acq_batch, 2100),
    ("ivar_grad", _ivar_grad, 300), ("var_grad_newpt", _var_grad_newpt, 300),
    ("lml_grad", _lml_grad, 300), ("mi_greedy", _mi_greedy, 300), ("greedy_var", _greedy_var, 300),
    ("dbg_greedy_var_scores", _dbg_greedy_var_scores, 300),
    ("loo", _loo, 300), ("loo_grad", _loo_grad, 300),
    ("fitc_fit+fitc_solve", _fitc, 300),
] + CHUNKED


@pytest.mark.parametrize("name,make,n", ENTRIES, ids=["%s-N%d" % (e[0], e[2]) for e in ENTRIES])
def test_outstanding_bytes_return_to_their_value(name, make, n):
    ctx, call = make(n)
    balanced(ctx, call)


@pytest.mark.parametrize("name,make,n", CHUNKED, ids=["%s-N%d" % (e[0], e[2]) for e in CHUNKED])
def test_outstanding_bytes_return_in_chunks_of_128(name, make, n, monkeypatch):
    ctx, call = make(n)
    monkeypatch.setenv("GPX_CROSS_BYTES", "1")
    balanced(ctx, call)


# ---- failure exits ---------------------------------------------------------------------------------------------------------------
BAD = -2.0   # as nugget / noise: the first pivot is 1.3 - 2 < 0 (or smaller still, behind a strip update)


def _refit_rows(n, keep):
    from gpexp_amd import device as dev
    ctx, spec, X, L, y, alpha, Z, Xh = model(n)

    def call(nugget):
        Lnew = dev.refit_rows(ctx, spec, X, nugget, L, keep)
        out = Lnew.to_host(tri=1)
        Lnew.free()
        return [out]
    return ctx, call


def _mi_greedy_noise(n):
    from gpexp_amd import device as dev
    ctx, spec, X, L, y, alpha, Z, Xh = model(n)
    return ctx, lambda noise: list(dev.mi_greedy(ctx, spec, Z, noise, 4))


def _mi_begin(n):
    from gpexp_amd import device as dev
    ctx, spec, X, L, y, alpha, Z, Xh = model(n)

    def call(noise):
        st = dev.MiState(ctx, spec, Z, noise, 4, 0, 0, M)
        rowbuf = dev.alloc_vector(ctx, M)
        st.row(0, rowbuf)
        val, idx = st.score(0, rowbuf)
        ctx.lib.gpx_mi_end(ctx.h, st.h)
        st.h = None
        rowbuf.free()
        return [np.array([val]), np.array([idx])]
    return ctx, call


def _fitc_fit(n):
    from gpexp_amd import device as dev
    ctx, spec, X, L, y, alpha, Z, Xh = model(n)

    def call(noise):
        S = dev.points(ctx, Xh[:64])
        try:
            f = dev.FitcModel(ctx, spec, X, S, noise)
            coeff, quad = f.solve(y)
            release(ctx, f)
        finally:
            S.free()
        return [coeff, np.array([quad])]
    return ctx, call


FAILURES = [
    ("refit_rows-N300-keep128", _refit_rows, (300, 128)), ("refit_rows-N4500-keep4096", _refit_rows, (4500, 4096)),
    ("mi_greedy-M260", _mi_greedy_noise, (300,)), ("mi_begin-M260", _mi_begin, (300,)),
    ("fitc_fit-N300-nu64", _fitc_fit, (300,)),
]


def digest(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def valid_digests():
    """Every case's VALID call, in case order, in a process that runs nothing else."""
    return {name: digest(make(*args)[1](NOISE)) for name, make, args in FAILURES}


@pytest.fixture(scope="module")
def fresh():
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][0][7:])


@pytest.mark.parametrize("name,make,args", FAILURES, ids=[f[0] for f in FAILURES])
def test_failure_exit_returns_its_scratch_and_leaves_the_entry_usable(name, make, args, fresh):
    from gpexp_amd._lib import GpxError
    ctx, call = make(*args)
    before = ctx.pool_stats()[1]
    with pytest.raises(GpxError) as err:
        call(BAD)
    after = ctx.pool_stats()[1]
    print("%s: %s\n    outstanding %d -> %d bytes" % (name, err.value, before, after))
    assert after == before, "the failed call left %d bytes of pool keys outstanding" % (after - before)
    got = digest(call(NOISE))
    print("    valid call afterwards %s, fresh process %s" % (got[:16], fresh[name][:16]))
    assert got == fresh[name]
    assert ctx.pool_stats()[1] == before
    assert ctx.guard_violations() <= 0   # 0 under GPX_ALLOC_GUARD=1, -1 with the guard off


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    print("RESULT " + json.dumps(valid_digests()))
