"""Element-wise accuracy of the covariance assembly (-m gpu): every entry the fill kernels write is held to the bound of
tests/kernel_reference.py against a 50-digit reference of the same function of the same doubles,

    |K_dev - k| <= (8 + e + 0.2 |x|) 2u |k| + D (2d + 16) u T + 2^-1073,

instead of max|a - b| / max|b|, which checks an entry of size 1e-9 to four digits.  Families (assembly section):
  a  kernel bodies and shapes: mirrored symmetric (diagonal, interior and ragged tiles), one-tile rectangular, the
     four-column-tile Matern kernel with a dead tile in its last group and with a single live tile
  b  operand widths K4 = 2, 3, 5, 9 at their boundaries d = 6|7, 10|11, 18|19, and d = 1, 32
  c  both distance forms, default selection and forced; the > 64 KiB LDS shapes of the Matern kernels in either form
  d  at the threshold between the forms, S * sens = 119 and 121
  e  every table index and exponent of the device exp, down to the denormal range and past it (exactly 0)
  f  offsets, signal sizes, per-point nugget
  g  kdiag, kernel_eval, kfill_into
  h  non-finite coordinates are refused, never turned into a finite covariance
Symmetric fills are also bit-symmetric, carry fl(sig + nugget) on the diagonal (stationary kinds) and write the identity --
and nothing else -- into their padding.
"""
import functools
import math
import os

import numpy as np
import pytest

import kernel_reference as kr
from oracle import gpexp_oracle as orc
from test_gpu_parity import spec_of

pytestmark = pytest.mark.gpu

STATIONARY = ("se", "matern32", "matern52")
ALL_KINDS = STATIONARY + ("mehler",)
FORMS = [None, "0", "1e300"]     # GPX_EXACT_S: default selection, differences forced, expanded product forced


def forms_of(kind):
    """Mehler has one form: the default run and one forced run that shows the switch is ignored."""
    return [None, "1e300"] if kind == "mehler" else FORMS


@pytest.fixture(scope="module")
def dev():
    from gpexp_amd import device
    return device


@pytest.fixture(scope="module")
def ctx(dev):
    return dev.context()


@pytest.fixture
def force_path():
    """GPX_EXACT_S is read per call: 0 forces raw differences, 1e300 forces the centred expanded product."""
    old = os.environ.get("GPX_EXACT_S")

    def set_(v):
        if v is None:
            os.environ.pop("GPX_EXACT_S", None)
        else:
            os.environ["GPX_EXACT_S"] = v
    yield set_
    set_(old)


# ---- cases: built once, shared ------------------------------------------------------------------------------------------------
def make_spec(kind, d, sig=1.3, ell=None):
    if kind == "se":
        cl = list(0.4 + 0.03 * np.arange(d)) if ell is None else [ell] * d
        return dict(kind="se", cl=cl, signalSize=sig, d=d)
    if kind == "mehler":
        return dict(kind="mehler", t=list(0.2 + 0.01 * np.arange(d)), d=d)
    return dict(kind=kind, rho=0.9 if ell is None else ell, signalSize=sig, d=d)


def sens_of(kind):
    return 1.0 / 6.0 if kind == "matern52" else 0.5


def scale_of(spec):
    hyp = kr.hyp_of(spec)
    if spec["kind"] == "se":
        return 1.0 / np.asarray(hyp[:spec["d"]])
    return np.full(spec["d"], math.sqrt(3.0 if spec["kind"] == "matern32" else 5.0) / hyp[0])


def default_half(kind, d):
    """Half-width that puts S * sens near 40 (the largest scale counted for every coordinate): well inside the expanded
    regime, far tails included (scaled diameters of ~9 sqrt(d / d) ... so exponents reach 40-80)."""
    if kind == "mehler":
        return 2.0
    c = float(np.max(scale_of(make_spec(kind, d))))
    return round(math.sqrt(40.0 / (sens_of(kind) * 2.0 * d)) / c, 3)


@functools.lru_cache(maxsize=None)
def case(kind, d, n, m, half=None, offset=0.0, sig=1.3, ell=None):
    spec = make_spec(kind, d, sig, ell)
    half = default_half(kind, d) if half is None else half
    X, Z = kr.structured_sets(spec, half, n, m, seed=7000 + 13 * d + n, offset=offset)
    X.setflags(write=False)
    Z.setflags(write=False)
    return spec, X, Z


@functools.lru_cache(maxsize=None)
def reference(symmetric, *key):
    spec, X, Z = case(*key)
    return kr.Reference(spec, X) if symmetric else kr.Reference(spec, X, Z)


def s_sens(spec, X, Z=None):
    """The library's S * sensitivity from the bounding box of the sets (api.hip, gpx_kparams_sets)."""
    P = X if Z is None else np.vstack([X, Z])
    lo, hi = P.min(0), P.max(0)
    hw = (hi - (0.5 * lo + 0.5 * hi)) * scale_of(spec)
    return float(np.sum(2.0 * hw * hw)) * sens_of(spec["kind"])


def expect_exact(spec, forced, X, Z=None):
    if spec["kind"] == "mehler":
        return False
    if forced is not None:
        return forced == "0"
    v = s_sens(spec, X, Z)
    assert abs(v - 120.0) > 0.5, "a case this close to the threshold must say which side it means"
    return v > 120.0


def nugget_of(n):
    return 0.01 + 0.003 * np.arange(n)


def raw_padded(ctx, K):
    """The whole padded storage of a device matrix, (prows, pcols)."""
    from gpexp_amd.device import C, c_i64, check, dptr
    r, c, ld = c_i64(), c_i64(), c_i64()
    check(ctx.lib.gpx_mat_shape(K.h, C.byref(r), C.byref(c), C.byref(ld)))
    prows = -(-max(r.value, 1) // 128) * 128
    pcols = -(-max(c.value, 1) // 128) * 128
    buf = np.empty(prows * ld.value)
    check(ctx.lib.gpx_mat_read(ctx.h, K.h, 0, buf.size, dptr(buf)))
    return buf.reshape(prows, ld.value)[:, :pcols]


def run_fill(dev, ctx, force_path, forced, key, symmetric, record=None):
    """One fill of the case `key`, checked against its bound; returns the worst error / bound."""
    spec, X, Z = case(*key)
    force_path(forced)
    ds = spec_of(dev, spec)
    dX = dev.points(ctx, X)
    dZ = None if symmetric else dev.points(ctx, Z)
    exact, center = dev.kfill_plan(ctx, ds, dX, dZ)
    assert exact == expect_exact(spec, forced, X, None if symmetric else Z)
    form = "diff" if exact else "expanded"
    ref = reference(symmetric, *key)
    label = "%s d=%d %s GPX_EXACT_S=%s" % (spec["kind"], spec["d"], "symmetric" if symmetric else "rectangular", forced)
    if symmetric:
        nug = nugget_of(len(X))
        Kd = dev.kfill(ctx, ds, dX, nugget=nug)
        K = Kd.to_host()
        r = ref.check(K, form, center, nugget=nug, label=label)
        assert np.array_equal(K, K.T), label + ": not bit-symmetric"
        if spec["kind"] != "mehler":
            assert np.array_equal(np.diag(K), spec["signalSize"] + nug), label + ": diagonal is not fl(sig + nugget)"
        P = raw_padded(ctx, Kd)
        n = len(X)
        assert np.array_equal(P[:n, :n], K)
        want = np.eye(P.shape[0])
        want[:n, :n] = K
        assert np.array_equal(P, want), label + ": padding is not the identity"
    else:
        Kd = dev.kfill(ctx, ds, dX, Z=dZ)
        K = Kd.to_host()
        r = ref.check(K, form, center, label=label)
        P = raw_padded(ctx, Kd)
        want = np.zeros(P.shape)
        want[:K.shape[0], :K.shape[1]] = K
        assert np.array_equal(P, want), label + ": padding is not zero"
    print("%s: %s form, worst error / bound = %.3f" % (label, form, r))
    return r, form, ref, K, center


# ---- a. shapes and kernel bodies ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,forced", [(kind, f) for kind in ALL_KINDS for f in forms_of(kind)])
def test_a_symmetric_n200(dev, ctx, force_path, kind, forced):
    """4 x 4 tile triangle: diagonal, interior and ragged edge tiles of the mirrored kernel."""
    run_fill(dev, ctx, force_path, forced, (kind, 3, 200, 70), True)


RECT = [("se", 130, 70), ("mehler", 130, 70),
        # outputs are padded to 128 columns = an even number of 64-column tiles:
        ("matern32", 70, 300), ("matern52", 70, 300),     # 384 = 6 tiles: a full group of 4, then 2 live + 2 dead
        ("matern32", 70, 64), ("matern52", 70, 64)]       # 128 = 2 tiles (the second all padding) + 2 dead


@pytest.mark.parametrize("kind,n,m,forced", [(kind, n, m, f) for kind, n, m in RECT for f in forms_of(kind)])
def test_a_rectangular(dev, ctx, force_path, kind, n, m, forced):
    run_fill(dev, ctx, force_path, forced, (kind, 3, n, m), False)


# ---- b, c. operand widths and distance forms ------------------------------------------------------------------------------
WIDTHS = [(kind, d) for d in (1, 7, 19, 32) for kind in ALL_KINDS]
WIDTHS += [(kind, d) for d in (6, 10, 11, 18) for kind in ("se", "matern32")]
# the operand images of the four-column-tile Matern kernel pass 64 KiB of LDS from d = 19 in the expanded form (covered above)
# and, with the difference form's stride of d | 1 doubles, from d = 24: one case just below that raise, two above
WIDTHS += [(kind, d) for d in (23, 24, 25) for kind in ("matern32", "matern52")]


@pytest.mark.parametrize("kind,d,forced", [(kind, d, f) for kind, d in WIDTHS for f in forms_of(kind)])
def test_bc_widths_and_forms(dev, ctx, force_path, kind, d, forced):
    """Symmetric n = 90 (3 tiles of the triangle, ragged) and rectangular 40 x 130 (256 padded columns: for the Matern kinds
    one full group of four column tiles, two of them ragged or all padding)."""
    run_fill(dev, ctx, force_path, forced, (kind, d, 90, 40), True)
    run_fill(dev, ctx, force_path, forced, (kind, d, 40, 130), False)


# ---- d. at the threshold between the forms --------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,ell", [("se", 0.2), ("matern52", 0.2582)])   # 5 / 0.2582^2 = 75.00 = 3 / 0.2^2
@pytest.mark.parametrize("half,exact", [(1.26, False), (1.27, True)])
def test_d_threshold(dev, ctx, force_path, kind, ell, half, exact):
    """d = 3: S * sens = 75 half^2 = 119.07 (expanded form) and 120.97 (differences).  The expanded case also meets the
    library's own figure for it, max|err| / sig <= 2e-14 (api.hip, exact_threshold)."""
    key = (kind, 3, 120, 40, half, 0.0, 1.3, ell)
    spec, X, Z = case(*key)
    assert abs(s_sens(spec, X) - 75.0 * half * half) < 0.01
    for symmetric in (True, False):
        r, form, ref, K, center = run_fill(dev, ctx, force_path, None, key, symmetric)
        assert form == ("diff" if exact else "expanded")
        if not exact:
            err = ref.max_error(K, nugget=nugget_of(len(X)) if symmetric else None)
            print("max|err| / sig at S * sens = %.2f: %.3g" % (s_sens(spec, X), err / spec["signalSize"]))
            assert err / spec["signalSize"] <= 2e-14


# ---- e. every table index, every exponent, the tails -----------------------------------------------------------------------
def sweep_arguments(far):
    m = np.concatenate([np.arange(4096), np.arange(4096 + 66, 275000, 67)])
    return np.concatenate([m * (math.log(2.0) / 256.0), far])


@functools.lru_cache(maxsize=None)
def sweep_case(kind, expanded):
    """X = [[0]], Z so that the exponent argument runs over m ln2 / 256: every j, n = 0 ... -15 densely, then to -745 and four
    points past it, where the value is below half a denormal step and must come out as exactly 0.  (The expanded run keeps
    those four close: its bound scales with the squared width of the set.  "Past it" starts where sig * poly(t) * e^-x drops
    under 2^-1075: x = 745.14 for SE with sig = 1, 745.28 for this Mehler kernel's sig = 1.155, t = 752.1 for Matern-3/2,
    whose factor 1 + t keeps the value on the denormal grid that much longer.)"""
    first = {"se": 745.2, "matern32": 753.0, "mehler": 745.5}[kind]
    far = np.array([first, first + 1.0, first + 7.0, 800.0] if expanded else [first, first + 7.0, 1e5, 1e9])
    arg = sweep_arguments(far)
    if kind == "se":
        spec, Z = dict(kind="se", cl=[1.0], signalSize=1.0, d=1), np.sqrt(2.0 * arg)
    elif kind == "matern32":
        spec, Z = dict(kind="matern32", rho=math.sqrt(3.0), signalSize=1.0, d=1), arg
    else:
        spec, Z = dict(kind="mehler", t=[0.5], d=1), np.sqrt(6.0 * arg)     # c1 = 1/6
    X = np.zeros((1, 1))
    Z = np.ascontiguousarray(Z.reshape(-1, 1))
    return spec, X, Z, kr.Reference(spec, X, Z)


@pytest.mark.parametrize("kind,forced", [("se", None), ("se", "1e300"), ("matern32", None), ("matern32", "1e300"),
                                         ("mehler", None)])
def test_e_exp_sweep(dev, ctx, force_path, kind, forced):
    expanded = forced == "1e300"
    spec, X, Z, ref = sweep_case(kind, expanded)
    force_path(forced)
    ds = spec_of(dev, spec)
    dX, dZ = dev.points(ctx, X), dev.points(ctx, Z)
    exact, center = dev.kfill_plan(ctx, ds, dX, dZ)
    assert exact == (kind != "mehler" and not expanded)    # 745 length scales wide: the default is the difference form
    K = dev.kfill(ctx, ds, dX, Z=dZ).to_host()
    r = ref.check(K, "diff" if exact else "expanded", center, label="exp sweep %s GPX_EXACT_S=%s" % (kind, forced))
    print("exp sweep %s GPX_EXACT_S=%s: worst error / bound = %.3f" % (kind, forced, r))
    assert np.all(K[0, -4:] == 0.0), K[0, -4:]
    assert np.all(K[0, :-4] > 0.0)
    assert kind == "mehler" or K[0, 0] == 1.0               # (Mehler's sig is a host pow(): within the bound, not pinned)
    assert np.all(np.diff(K[0]) <= 0.0)                     # monotone through every table / exponent step
    # the sweep reached what it is for: denormal results, and every table index (m = 0 ... 4095 are consecutive)
    assert np.sum((K[0] > 0.0) & (K[0] < 2.0 ** -1022)) > 100
    # the transposed call takes the other operand side and the ragged row tiles
    Kt = dev.kfill(ctx, ds, dZ, Z=dX).to_host()
    ref.check(Kt.T, "diff" if exact else "expanded", center, label="exp sweep (transposed) %s" % kind)


# ---- f. offsets and scales ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("forced", FORMS)
@pytest.mark.parametrize("offset", [1.0e3, -3.0e4])
@pytest.mark.parametrize("kind", ["se", "matern52"])
def test_f_offsets(dev, ctx, force_path, kind, offset, forced):
    """The structured set far from the origin.  Both forms subtract before they scale (the expanded one the centre), so the
    bound -- a function of the centred operands only -- holds wherever the set sits."""
    key = (kind, 3, 90, 40, None, offset)
    run_fill(dev, ctx, force_path, forced, key, True)
    run_fill(dev, ctx, force_path, forced, key, False)


@pytest.mark.parametrize("sig", [1e-6, 1e6])     # 1.3 is every other case
@pytest.mark.parametrize("kind", STATIONARY)
def test_f_signal_size(dev, ctx, force_path, kind, sig):
    for forced in FORMS:
        key = (kind, 3, 90, 40, None, 0.0, sig)
        run_fill(dev, ctx, force_path, forced, key, True)
        run_fill(dev, ctx, force_path, forced, key, False)


def test_f_scalar_and_absent_nugget(dev, ctx, force_path):
    """(Every symmetric case above carries a per-point nugget array.)"""
    key = ("se", 3, 90, 40)
    spec, X, Z = case(*key)
    ref = reference(True, *key)
    ds, dX = spec_of(dev, spec), dev.points(ctx, X)
    exact, center = dev.kfill_plan(ctx, ds, dX)
    form = "diff" if exact else "expanded"
    K0 = dev.kfill(ctx, ds, dX).to_host()
    ref.check(K0, form, center)
    K1 = dev.kfill(ctx, ds, dX, nugget=0.37).to_host()
    ref.check(K1, form, center, nugget=0.37)
    assert np.array_equal(np.diag(K0), np.full(len(X), spec["signalSize"]))
    assert np.array_equal(np.diag(K1), np.full(len(X), spec["signalSize"] + 0.37))
    off = ~np.eye(len(X), dtype=bool)
    assert np.array_equal(K0[off], K1[off])


# ---- g. other evaluators of the same function -----------------------------------------------------------------------------
@pytest.mark.parametrize("kind,d", [(kind, d) for kind in ALL_KINDS for d in (3, 19)])
def test_g_kdiag_and_kernel_eval(dev, ctx, kind, d):
    spec, X, Z = case(kind, d, 90, 40)
    ds = spec_of(dev, spec)
    n = len(X)
    I = np.arange(n)
    ref = kr.Reference(spec, X, X, pairs=(I, I))
    r0 = ref.check(dev.kdiag(ctx, ds, dev.points(ctx, X)), "diff", label="kdiag %s" % kind)
    J = I[::-1].copy()
    J[0:5] = I[10:15]       # a point and its exact duplicate
    J[10:15] = I[15:20]     # a point and its neighbour at 1e-9 ... 1e-1
    ref = kr.Reference(spec, X, X, pairs=(I, J))
    r1 = ref.check(dev.kernel_eval(ctx, ds, X, X[J]), "diff", label="kernel_eval paired %s" % kind)
    # one against n: row 0 has an exact duplicate (row 10) and the 1e-9 neighbour (row 15)
    ref = kr.Reference(spec, X, X, pairs=(I, np.zeros(n, dtype=int)))
    r2 = ref.check(dev.kernel_eval(ctx, ds, X, X[:1]), "diff", label="kernel_eval n vs 1 %s" % kind)
    r3 = ref.check(dev.kernel_eval(ctx, ds, X[:1], X), "diff", label="kernel_eval 1 vs n %s" % kind)
    print("%s d=%d: kdiag %.3f, kernel_eval paired %.3f, n-vs-1 %.3f, 1-vs-n %.3f" % (kind, d, r0, r1, r2, r3))


@pytest.mark.parametrize("kind", ["se", "matern32", "mehler"])
def test_g_kfill_into_padded(dev, ctx, kind):
    """kfill_into a padded matrix that held something else: the logical block is kfill's bit for bit, the padding is the
    identity (symmetric) / zero (rectangular) -- nothing of the old contents, nothing of the staged zero points."""
    from gpexp_amd.device import check, dptr
    spec, X, Z = case(kind, 3, 200, 70)
    ds = spec_of(dev, spec)
    dX, dZ = dev.points(ctx, X), dev.points(ctx, Z)
    nug = nugget_of(len(X))
    for Zd, rows, cols in ((None, 200, 200), (dZ, 200, 70)):
        K = dev.DeviceMatrix.zeros(ctx, rows, cols, pad=True)
        poison = np.full(raw_padded(ctx, K).shape, 7.25)
        assert poison.shape[1] < 1024   # no skew columns: the raw storage is exactly (prows, pcols)
        check(ctx.lib.gpx_mat_write(ctx.h, K.h, 0, poison.size, dptr(poison)))
        if Zd is None:
            dev.kfill_into(ctx, ds, dX, K, nugget=nug)
            want_logical = dev.kfill(ctx, ds, dX, nugget=nug).to_host()
            want = np.eye(poison.shape[0])
        else:
            dev.kfill_into(ctx, ds, dX, K, Z=Zd)
            want_logical = dev.kfill(ctx, ds, dX, Z=Zd).to_host()
            want = np.zeros(poison.shape)
        assert np.array_equal(K.to_host(), want_logical)
        want[:rows, :cols] = want_logical
        assert np.array_equal(raw_padded(ctx, K), want)


# ---- h. non-finite coordinates --------------------------------------------------------------------------------------------
def nonfinite_outcome(dev, ctx, spec, X, Z):
    """Runs the fill; returns None when the library refused the set by name, else the matrix."""
    from gpexp_amd._lib import GpxError
    ds = spec_of(dev, spec)
    try:
        dX = dev.points(ctx, X)
        if Z is None:
            return dev.kfill(ctx, ds, dX, nugget=0.05).to_host()
        return dev.kfill(ctx, ds, dX, Z=dev.points(ctx, Z)).to_host()
    except GpxError as e:
        assert "non-finite" in str(e) and "row 37, column 1" in str(e), str(e)
        return None


@pytest.mark.parametrize("bad", [np.nan, np.inf])
@pytest.mark.parametrize("symmetric", [True, False])
@pytest.mark.parametrize("kind", ["se", "matern32"])
def test_h_nonfinite_coordinate(dev, ctx, kind, symmetric, bad):
    """A pair that involves a NaN coordinate never yields a finite number: the call is refused with an error that names the
    non-finite coordinate, or those entries are NaN and the rest meets the bound.  For an infinity: the same error, or NumPy's
    values under the oracle's formula."""
    spec, X, Z = case(kind, 3, 90, 40)
    X = X.copy()
    X[37, 1] = bad
    K = nonfinite_outcome(dev, ctx, spec, X, None if symmetric else Z)
    if K is None:
        # the refusal is of that set alone: the clean sets still go through, and the bad one is refused as Z too
        from gpexp_amd._lib import GpxError
        ds = spec_of(dev, spec)
        good = case(kind, 3, 90, 40)[1]
        dev.kfill(ctx, ds, dev.points(ctx, good))
        with pytest.raises(GpxError, match="non-finite"):
            dev.kfill(ctx, ds, dev.points(ctx, good), Z=dev.points(ctx, X))
        return
    with np.errstate(invalid="ignore"):
        want = orc.cov_matrix(spec, X, 0.05, row_loop=False) if symmetric else orc.cross_matrix(spec, Z, X).T
    involved = np.zeros(K.shape, dtype=bool)
    involved[37, :] = True
    if symmetric:
        involved[:, 37] = True
    if np.isnan(bad):
        assert np.all(np.isnan(K[involved])), "a pair with a NaN coordinate came out finite"
    else:
        assert np.array_equal(np.isnan(K[involved]), np.isnan(want[involved]))
        fin = involved & ~np.isnan(want)
        assert np.array_equal(K[fin], want[fin])
    ref = reference(symmetric, kind, 3, 90, 40)
    keep = ~involved[ref.I, ref.J]
    exact, center = dev.kfill_plan(ctx, spec_of(dev, spec), dev.points(ctx, X))
    r = ref.ratios(K, "diff" if exact else "expanded", center, nugget=0.05 if symmetric else None)
    assert np.all(r[keep] <= 1.0)


def test_h_slice_with_the_box_of_the_whole_set(dev, ctx):
    """points_slice (gpx_points_set_box) keeps working, and a box given by the caller does not hide a NaN in the slice."""
    from gpexp_amd._lib import GpxError
    spec, X, Z = case("se", 3, 90, 40)
    ds = spec_of(dev, spec)
    dX = dev.points(ctx, X)
    whole = dev.kfill(ctx, ds, dX, Z=dev.points(ctx, Z)).to_host()
    part = dev.kfill(ctx, ds, dX, Z=dev.points_slice(ctx, np.vstack([X, Z]), 90 + 8, 90 + 30)).to_host()
    assert np.array_equal(part, whole[:, 8:30])      # the slice carries the box of X and Z: same centre, same bits
    from gpexp_amd.device import check, dptr
    bad = Z[8:30].copy()
    bad[4, 2] = np.nan
    dS = dev.points(ctx, bad)
    lo, hi = np.ascontiguousarray(X.min(0)), np.ascontiguousarray(X.max(0))
    check(ctx.lib.gpx_points_set_box(ctx.h, dS.h, dptr(lo), dptr(hi), 3))
    with pytest.raises(GpxError, match="non-finite.*row 4, column 2"):
        dev.kfill(ctx, ds, dX, Z=dS)


def test_h_gp_train_with_a_nan_point(dev, ctx):
    from gpexp_amd._lib import GpxError
    from gpexp_amd.gp import GP
    from gpexp_amd.kernels import KernelSquaredExponential
    rng = np.random.default_rng(3)
    X = rng.uniform(-1, 1, (60, 2))
    y = np.sin(X.sum(1))
    X[11, 0] = np.nan
    gp = GP(KernelSquaredExponential([0.5, 0.5], 1.0, 2), 0.05)
    try:
        gp.train(X, y)
    except (GpxError, ValueError, FloatingPointError):
        return
    assert np.all(np.isnan(np.asarray(gp.coeff, dtype=float))), "a GP trained on a NaN point in silence"
