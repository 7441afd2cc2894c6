"""High-precision restatement of the four covariance functions and the element-wise error bound the assembly is held to.

Inputs are the doubles the device gets: the points, the hyper-parameters and (for the expanded distance form) the centre
the library subtracts (`device.kfill_plan`).  The true value of every pair comes out of the standard library's `decimal`
at 50 digits (`Decimal(float)` is exact, `.exp()` and `.sqrt()` are correctly rounded), so nothing beyond NumPy is needed.

With u = 2^-53, per pair (a, b):

  stationary kinds   scale_k = 1/cl_k (SE), sqrt(3)/rho (Matern-3/2), sqrt(5)/rho (Matern-5/2), formed in high precision
                     from the double hyper-parameter;  s = sum_k ((a_k - b_k) scale_k)^2
      SE          x = s/2         k = sig e^-x                  D = |dk/ds| = k/2
      Matern-3/2  x = t = sqrt s  k = sig (1 + t) e^-t          D = sig e^-t / 2
      Matern-5/2  x = t = sqrt s  k = sig (1 + t + s/3) e^-t    D = sig (1 + t) e^-t / 6
    distance term T: difference form  T = s
                     expanded form    a' = (a - c) scale, b' = (b - c) scale, T = |a'|^2 + |b'|^2 + 2 sum_k |a'_k b'_k|
  Mehler             x = sum_k c1_k (a_k^2 + b_k^2) - c2_k a_k b_k,  k = sig e^-x,  D = k,
                     T = sum_k c1_k (a_k^2 + b_k^2) + |c2_k a_k b_k|
                     sig = prod (1 - t_k^2)^-1/2, c1_k = t_k^2 / (2 (1 - t_k^2)), c2_k = t_k / (1 - t_k^2)

  bound = (8 + e + 0.2 |x|) 2u |k|  +  D (2d + 16) u T  +  2^-1073        e = 3d for Mehler (the host's product for sig), else 0

  0.2 |x|        the growth of the device exp's error with its argument: the one-constant range reduction leaves
                 m (C - ln2/256); measured 0.155 |x| units of 2^-52 (tests/test_kernel_reference_host.py), rounded up
  8              table entry, polynomial, tj * p, sqrt, the polynomial factor of the Matern kinds, the product with sig
  (2d + 16) u T  the dot-product bound gamma_K sum |a'_k b'_k| of the K = d + 2 augmented operand, two roundings per step in
                 case the matrix pipe does not fuse, plus at most 5u per staged coordinate (x - c, * scale, the rounding of
                 scale itself)
  2^-1073        one step of the denormal grid

  On the diagonal of a symmetric fill with a nugget the true value is k + nugget and the bound gains u |k + nugget|, the one
  rounding of that sum (fl(sig + nugget) with sig = 1e-6 cannot be within 16 u sig of it); see Reference.errors.

The constants are derived, not tuned: a case over the bound is a finding about the kernel, not about the bound.
"""
import decimal
from decimal import Decimal

import numpy as np

PREC = 50
U = 2.0 ** -53
DENORMAL_STEP = 2.0 ** -1073
STATIONARY = ("se", "matern32", "matern52")

_CTX = decimal.Context(prec=PREC, rounding=decimal.ROUND_HALF_EVEN, Emin=-999999999, Emax=999999999,
                       traps=[decimal.InvalidOperation, decimal.DivisionByZero, decimal.Overflow])
_ZERO = Decimal(0)
_ONE = Decimal(1)
_FAR = Decimal(1200)  # e^-1200 = 1e-521: nothing a double can tell from 0, and no need to evaluate it


def hyp_of(spec):
    """The flat hyper-parameter doubles the device is given (tests: test_gpu_parity.spec_of)."""
    kind, d = spec["kind"], spec["d"]
    if kind == "se":
        cl = np.asarray(spec["cl"], dtype=float).ravel()
        if cl.size == 1:
            cl = np.tile(cl, d)
        return [float(v) for v in cl] + [float(spec["signalSize"])]
    if kind in ("matern32", "matern52"):
        return [float(spec["rho"]), float(spec["signalSize"])]
    if kind == "mehler":
        return [float(t) for t in spec["t"]]
    raise ValueError("unknown kernel kind %r" % (kind,))


def _params(spec):
    """(sig, scale[d], c1[d], c2[d]) as Decimals, from the double hyper-parameters."""
    kind, d = spec["kind"], spec["d"]
    hyp = [Decimal(v) for v in hyp_of(spec)]
    with decimal.localcontext(_CTX):
        if kind == "se":
            return hyp[d], [_ONE / hyp[k] for k in range(d)], None, None
        if kind == "matern32":
            return hyp[1], [Decimal(3).sqrt() / hyp[0]] * d, None, None
        if kind == "matern52":
            return hyp[1], [Decimal(5).sqrt() / hyp[0]] * d, None, None
        sig, c1, c2 = _ONE, [], []
        for t in hyp:
            om = _ONE - t * t
            c1.append(t * t / (2 * om))
            c2.append(t / om)
            sig = sig / om.sqrt()
        return sig, [_ONE] * d, c1, c2


def _dec_rows(P):
    return [[Decimal(float(v)) for v in row] for row in np.asarray(P, dtype=float)]


class Reference:
    """True kernel values and bounds for pairs (A[I[p]], B[J[p]]).

    B None: the symmetric fill of A, pairs = the lower triangle with the diagonal (the default `pairs`).
    B given: every pair of the rectangle unless `pairs = (I, J)` says otherwise.
    """

    def __init__(self, spec, A, B=None, pairs=None):
        self.spec = dict(spec)
        self.kind, self.d = spec["kind"], int(spec["d"])
        self.A = np.ascontiguousarray(A, dtype=float)
        self.sym = B is None
        self.B = self.A if B is None else np.ascontiguousarray(B, dtype=float)
        assert self.A.ndim == 2 and self.B.ndim == 2 and self.A.shape[1] == self.d and self.B.shape[1] == self.d
        if pairs is None:
            if self.sym:
                I, J = np.tril_indices(self.A.shape[0])
            else:
                I, J = np.indices((self.A.shape[0], self.B.shape[0]))
        else:
            I, J = pairs
        self.I = np.asarray(I, dtype=np.int64).ravel()
        self.J = np.asarray(J, dtype=np.int64).ravel()
        self._evaluate()

    # -- the true values ------------------------------------------------------------------------------------------------
    def _evaluate(self):
        kind, d = self.kind, self.d
        sig, sc, c1, c2 = _params(self.spec)
        self.sig = float(sig)
        Ad = _dec_rows(self.A)
        Bd = Ad if self.sym else _dec_rows(self.B)
        n = self.I.size
        k_out = [None] * n
        x_out = np.empty(n)
        D_out = [None] * n
        T_out = np.empty(n)
        rng_d = range(d)
        three, two, six = Decimal(3), Decimal(2), Decimal(6)
        with decimal.localcontext(_CTX):
            for p in range(n):
                a, b = Ad[self.I[p]], Bd[self.J[p]]
                if kind == "mehler":
                    x, T = _ZERO, _ZERO
                    for k in rng_d:
                        q = c1[k] * (a[k] * a[k] + b[k] * b[k])
                        c = c2[k] * a[k] * b[k]
                        x += q - c
                        T += q + abs(c)
                    kv = sig * (-x).exp() if x < _FAR else _ZERO
                    D = kv
                else:
                    s = _ZERO
                    for k in rng_d:
                        e = (a[k] - b[k]) * sc[k]
                        s += e * e
                    T = s
                    if kind == "se":
                        x = s / two
                        kv = sig * (-x).exp() if x < _FAR else _ZERO
                        D = kv / two
                    else:
                        x = s.sqrt()
                        ex = (-x).exp() if x < _FAR else _ZERO
                        if kind == "matern32":
                            kv = sig * (_ONE + x) * ex
                            D = sig * ex / two
                        else:
                            kv = sig * (_ONE + x + s / three) * ex
                            D = sig * (_ONE + x) * ex / six
                k_out[p] = kv
                x_out[p] = float(x)
                D_out[p] = D
                T_out[p] = float(T)
        self.k = k_out
        self.kf = np.array([float(v) for v in k_out])
        self.x, self.D, self.T_diff = x_out, D_out, T_out
        self._scale = np.array([float(v) for v in sc])

    # -- the bound ------------------------------------------------------------------------------------------------------
    def expanded_T(self, center):
        """|a'|^2 + |b'|^2 + 2 sum |a'_k b'_k| of the centred, scaled operands (float64: it only scales a bound)."""
        c = np.asarray(center, dtype=float)
        a = np.abs((self.A - c[None, :]) * self._scale[None, :])[self.I]
        b = np.abs((self.B - c[None, :]) * self._scale[None, :])[self.J]
        return np.sum(a * a, axis=1) + np.sum(b * b, axis=1) + 2.0 * np.sum(a * b, axis=1)

    def bound(self, form="diff", center=None):
        """Per pair, as Decimals (in float64 the products underflow for values in the denormal range, where the bound is a few
        grid steps).  form: 'diff' (coordinate differences; also Mehler, which has one form) or 'expanded' (needs `center`)."""
        if self.kind == "mehler" or form == "diff":
            T = self.T_diff
        elif form == "expanded":
            assert center is not None, "the expanded form's bound needs the centre the device used"
            T = self.expanded_T(center)
        else:
            raise ValueError(form)
        e = 3.0 * self.d if self.kind == "mehler" else 0.0
        rel = (8.0 + e + 0.2 * np.abs(self.x)) * 2.0 * U
        dot = (2.0 * self.d + 16.0) * U * T
        step = Decimal(DENORMAL_STEP)
        with decimal.localcontext(_CTX):
            return [Decimal(float(rel[p])) * abs(self.k[p]) + self.D[p] * Decimal(float(dot[p])) + step
                    for p in range(len(self.k))]

    # -- comparing ------------------------------------------------------------------------------------------------------
    def _pick(self, values):
        v = np.asarray(values, dtype=float)
        if v.ndim == 2:
            return v[self.I, self.J]
        assert v.shape == self.I.shape, "a vector of values must have one entry per pair"
        return v

    def errors(self, values, nugget=None):
        """(|value - true| per pair, extra bound per pair), as Decimals.  `nugget` (scalar or one per point) is what a symmetric fill added
        to its diagonal: the true value there is k + nugget and the one rounding of that sum, u |k + nugget|, is allowed."""
        v = self._pick(values)
        err = [None] * v.size
        extra = [_ZERO] * v.size
        nug = None
        if nugget is not None:
            assert self.sym
            nug = np.broadcast_to(np.asarray(nugget, dtype=float), (self.A.shape[0],))
        with decimal.localcontext(_CTX):
            for p in range(v.size):
                if not np.isfinite(v[p]):
                    err[p] = Decimal("Infinity")
                    continue
                want = self.k[p]
                if nug is not None and self.I[p] == self.J[p]:
                    want = want + Decimal(float(nug[self.I[p]]))
                    extra[p] = Decimal(U) * abs(want)
                err[p] = abs(Decimal(float(v[p])) - want)
        return err, extra

    def max_error(self, values, nugget=None):
        """max |value - true| as a float."""
        return float(max(self.errors(values, nugget)[0]))

    def ratios(self, values, form="diff", center=None, nugget=None):
        err, extra = self.errors(values, nugget)
        bound = self.bound(form, center)
        with decimal.localcontext(_CTX):
            return np.array([float(err[p] / (bound[p] + extra[p])) for p in range(len(err))])

    def worst(self, values, form="diff", center=None, nugget=None):
        """(largest error / bound, description of that pair)."""
        r = self.ratios(values, form, center, nugget)
        p = int(np.argmax(r))
        v = self._pick(values)
        what = ("pair (%d, %d): x = %.17g, value = %.17g, reference = %.17g, error / bound = %.4g"
                % (self.I[p], self.J[p], self.x[p], v[p], self.kf[p], r[p]))
        return float(r[p]), what

    def failures(self, values, form="diff", center=None, nugget=None):
        """Index pairs (i, j) whose error exceeds the bound."""
        r = self.ratios(values, form, center, nugget)
        bad = np.nonzero(~(r <= 1.0))[0]
        return [(int(self.I[p]), int(self.J[p])) for p in bad]

    def check(self, values, form="diff", center=None, nugget=None, label=""):
        """Assert max error / bound <= 1; the message names the worst pair.  Returns the worst ratio."""
        r, what = self.worst(values, form, center, nugget)
        assert r <= 1.0, "%s over the bound (%s form): %s" % (label or self.kind, form, what)
        return r


# ---- the structured point sets of the accuracy tests ----------------------------------------------------------------------
def structured_sets(spec, half, n, m, seed, offset=0.0):
    """X (n, d) and Z (m, d) in the box offset +- half:
      * uniform points;
      * 5 exact duplicates within X, and 5 rows of Z equal to rows of X;
      * 5 neighbours (in X and in Z, of rows of X) at 1e-9, 1e-7, 1e-5, 1e-3, 1e-1 SCALED distance;
      * the two opposite corners offset -+ half in every coordinate as the last two rows of X: the bounding box is exact.
    """
    d = spec["d"]
    assert n >= 24 and m >= 12
    rng = np.random.default_rng(seed)
    hyp = hyp_of(spec)
    if spec["kind"] == "se":
        scale = 1.0 / np.asarray(hyp[:d])
    elif spec["kind"] == "matern32":
        scale = np.full(d, np.sqrt(3.0) / hyp[0])
    elif spec["kind"] == "matern52":
        scale = np.full(d, np.sqrt(5.0) / hyp[0])
    else:
        scale = np.ones(d)
    X = rng.uniform(-half, half, (n, d))
    Z = rng.uniform(-half, half, (m, d))
    # sources are drawn from a shrunken box so that a neighbour cannot leave the box
    src = rng.uniform(-0.8 * half, 0.8 * half, (10, d))
    X[:10] = src
    X[10:15] = src[:5]                     # duplicates within X (rows 10..14 == rows 0..4)
    Z[:5] = src[5:10]                      # rows of Z equal to rows of X
    dists = [1e-9, 1e-7, 1e-5, 1e-3, 1e-1]
    for q, dist in enumerate(dists):
        u = rng.standard_normal(d)
        u /= np.linalg.norm(u)
        X[15 + q] = src[q] + dist * u / scale
        u = rng.standard_normal(d)
        u /= np.linalg.norm(u)
        Z[5 + q] = src[q] + dist * u / scale
    np.clip(X, -half, half, out=X)
    np.clip(Z, -half, half, out=Z)
    X[n - 2] = -half
    X[n - 1] = half
    return X + offset, Z + offset
