"""CPU: pins the references, metrics and comparators tests/test_gpu_posterior_bounds.py judges the device by, before the device is
judged by them (tests/posterior_ref.py).

The longdouble reference agrees with a 50-digit `decimal` evaluation on a 12-point case; the refined, sampled reference of the
large case agrees with the full route; the comparators (LAPACK, the b = 128 explicit-inverse emulation) score O(1 .. 10) in the
per-point metric whatever cond(K); every mutant -- a comparator route with one defect -- is rejected by the bound rule with a factor
of ten to spare; and the max-norm metric of the older posterior tests lets a defect through that the per-point metric rejects.
Run with -s for the figures.

Measured here (fp64 LAPACK / b128; cond(K) 1.5e3 .. 7e7): omega_v 1.7 .. 8.0 / 2.4 .. 12.6, omega_m 0.3 .. 1.2, omega_M 0.1 .. 0.9 /
0.1 .. 4.5, omega_I <= 0.15, omega_c 3.2 .. 8.9 / 3.0 .. 76.9 (the explicit inverses' W is not componentwise backward stable off the
diagonal of the covariance: se-tiny-noise 76.9, m52-tiny-noise 22.2).  The 3e-13 scaling of B scores omega_v 6.4e2 .. 1.4e3 and
max-norm 6.6e-12 (se-well): it passes `rel <= 1e-10`.  The three structural mutants (last row, row chunk, tile seam) do NOT pass
`rel <= 1e-10` on any case drawn here (smallest: 7.2e-4, 2.2e1 and 1.8e-1): with 300 points in [-1, 1]^3 every variance is small and
every training row matters to some point; they are rejected by both metrics, by omega with 1e8 .. 1e15."""
import decimal
from decimal import Decimal

import numpy as np
import pytest

import design_replay_ref as DR
import kernel_reference as KR
import posterior_ref as P

LD = P.LD


@pytest.fixture(scope="module")
def refs():
    """name -> (arrays, reference, comparator omegas), built once per case."""
    cache = {}

    def get(name):
        if name not in cache:
            c = P.case(name)
            K, B, kd, kzz = P.host_arrays(name)
            al = P.host_alpha(name)
            ref = P.reference(K, B, kd, c["y"], al, kzz)
            cache[name] = ((K, B, kd, kzz, al), ref, P.comparator_omegas(ref, K, B, kd, c["y"], al, kzz))
        return cache[name]
    return get


def test_case_layout():
    for name in P.CASES:
        c = P.case(name)
        X, Z, n = c["X"], c["Z"], c["n"]
        assert Z.shape == (P.M_EVAL, 3) and not Z.flags.writeable and not X.flags.writeable
        assert [int(np.nonzero((X == z).all(axis=1))[0][0]) for z in Z[:4]] == [0, 127, 128, n - 1]
        for z in Z[:P.N_ON]:
            assert (X == z).all(axis=1).sum() == 1
        dist = np.min(np.linalg.norm(X[None, :, :] - Z[P.N_ON:P.N_ON + P.N_NEAR, None, :], axis=2), axis=1)
        assert np.all((dist > 0) & (dist < 1e-6)), dist
        assert np.min(np.linalg.norm(X[None, :, :] - Z[P.N_ON + P.N_NEAR:, None, :], axis=2)) > 1e-4
        # the moved rows keep the bounding box: a refit that keeps leading rows sees the fills it kept
        assert np.array_equal(X.min(axis=0), c["X2"].min(axis=0)) and np.array_equal(X.max(axis=0), c["X2"].max(axis=0))
        assert np.array_equal(X[:n - P.MOVED], c["X2"][:n - P.MOVED]) and not np.any(X[n - P.MOVED:] == c["X2"][n - P.MOVED:])
    nug = P.case("m32-per-point")["nugget"]
    assert nug.shape == (300,) and nug.min() >= 1e-6 and nug.max() <= 1e-2 and nug.max() / nug.min() > 1e3
    assert set(P.sampled_cols()) >= {0, 1, 2, 3, P.N_ON, P.N_ON + 1} and P.sampled_cols().size == P.N_SAMPLED


# ---- the reference against 50 digits ------------------------------------------------------------------------------------------
_CTX = decimal.Context(prec=50)


def _dec_reference(K, B, kd, y, alpha, kzz):
    """v, m, M, c of float64 arrays by a Cholesky factorisation in 50-digit decimal arithmetic."""
    n, m = B.shape
    with decimal.localcontext(_CTX):
        Kd = [[Decimal(float(v)) for v in row] for row in K]
        L = [[Decimal(0)] * n for _ in range(n)]
        for j in range(n):
            L[j][j] = (Kd[j][j] - sum(L[j][k] * L[j][k] for k in range(j))).sqrt()
            for i in range(j + 1, n):
                L[i][j] = (Kd[i][j] - sum(L[i][k] * L[j][k] for k in range(j))) / L[j][j]

        def fwd(b):
            w = []
            for i in range(n):
                w.append((b[i] - sum(L[i][k] * w[k] for k in range(i))) / L[i][i])
            return w

        def bwd(w):
            x = [Decimal(0)] * n
            for i in range(n - 1, -1, -1):
                x[i] = (w[i] - sum(L[k][i] * x[k] for k in range(i + 1, n))) / L[i][i]
            return x

        Bd = [[Decimal(float(B[i, j])) for i in range(n)] for j in range(m)]
        W = [fwd(b) for b in Bd]
        ah = bwd(fwd([Decimal(float(v)) for v in y]))
        v = [Decimal(float(kd[j])) - sum(x * x for x in W[j]) for j in range(m)]
        mg = [sum(Bd[j][i] * Decimal(float(alpha[i])) for i in range(n)) for j in range(m)]
        Me = [sum(Bd[j][i] * ah[i] for i in range(n)) for j in range(m)]
        c = [[Decimal(float(kzz[j, l])) - sum(W[j][i] * W[l][i] for i in range(n)) for l in range(m)] for j in range(m)]
    return v, mg, Me, c


def test_reference_against_fifty_digits():
    """12 training points, 5 evaluation points (one on a training point, one 1e-7 from one), noise 1e-6: every value of the longdouble
    reference within 2^-58 of the 50-digit one, in units of the metric's own scale S (u S = 2^-53 S is what omega counts in: the
    reference is 32 times finer on a case of cond 1e6)."""
    rng = np.random.default_rng(12)
    X = rng.uniform(-1.0, 1.0, (12, 3))
    Z = np.vstack([X[3], X[7] + 1e-7 * rng.standard_normal(3), rng.uniform(-1.0, 1.0, (3, 3))])
    K = DR.cov_f64(P.SE3, X)
    K = 0.5 * (K + K.T) + 1e-6 * np.eye(12)
    B, kzz = DR.cov_f64(P.SE3, X, Z), DR.cov_f64(P.SE3, Z)
    kzz = 0.5 * (kzz + kzz.T)
    kd, y = np.diag(kzz).copy(), rng.standard_normal(12)
    alpha = np.linalg.solve(K, y)
    ref = P.reference(K, B, kd, y, alpha, kzz)
    v, mg, Me, c = _dec_reference(K, B, kd, y, alpha, kzz)
    worst = {}
    for key, dec in (("v", v), ("m", mg), ("M", Me), ("c", [x for row in c for x in row])):
        got = np.ravel(ref["val"][key])
        scale = np.ravel(ref["scale"][key])
        with decimal.localcontext(_CTX):
            err = [abs(Decimal(float(got[i])) + Decimal(float(got[i] - LD(float(got[i])))) - dec[i]) for i in range(got.size)]
            worst[key] = max(float(err[i] / Decimal(float(scale[i]))) for i in range(got.size))
    print("\nreference against 50 digits, error / S: %s   (2^-58 = %.2e; cond %.1e)"
          % ("  ".join("%s %.2e" % kv for kv in worst.items()), 2.0 ** -58, np.linalg.cond(K)))
    for key, w in worst.items():
        assert w <= 2.0 ** -58, (key, w)


@pytest.mark.parametrize("name", P.SMALL)
def test_sampled_reference_equals_the_full_route(name, refs):
    """The full route is the float64 algorithm with 11 more bits, so its own error in units of u S is about omega_v(LAPACK) 2^-11;
    the sampled route's is below 1e-5 (its residual is under 2^-60 |b| by construction and beta^T r is all that is left).  The two
    are held together to 1e-3 where the full route itself is that good -- `mehler`, omega_v(LAPACK) = 1.7, the smallest of the
    cases -- and to twice the full route's predicted error, omega_v(LAPACK) 2^-10, everywhere (measured 7.6e-4 .. 2.2e-3)."""
    (K, B, kd, _, _), ref, cmp_ = refs(name)
    cols = P.sampled_cols()
    rs = P.reference_sampled(K, B, kd, cols)
    assert np.all(np.max(np.abs(rs["residual"]), axis=0).astype(float) <= 2.0 ** -60 * np.max(np.abs(B[:, cols]), axis=0))
    diff = float(np.max(np.abs(rs["val"]["v"] - ref["val"]["v"][cols]) / (LD(P.U) * rs["scale"]["v"])))
    assert np.allclose(rs["scale"]["v"], ref["scale"]["v"][cols], rtol=1e-9, atol=0.0)
    print("\n%-16s sampled - full = %.2e u S   (omega_v LAPACK %.2f -> 2^-10 x = %.2e)"
          % (name, diff, cmp_["v"]["lapack"], cmp_["v"]["lapack"] * 2.0 ** -10))
    assert diff <= cmp_["v"]["lapack"] * 2.0 ** -10
    if name == "mehler":
        assert diff <= 1e-3


def test_sampled_reference_of_the_large_case():
    """n = 2200: the refinement reaches its residual, and the comparators score on the sampled columns what they score at n = 300."""
    K, B, kd, _ = P.host_arrays("m52-oop")
    cols = P.sampled_cols()
    rs = P.reference_sampled(K, B, kd, cols)
    cmp_ = P.comparator_omegas(rs, K, B, kd, cols=cols)
    print("\nm52-oop cond %.1e  omega_v %s" % (np.linalg.cond(K), cmp_["v"]))
    assert max(cmp_["v"].values()) <= 16.0, cmp_


# ---- the comparators and the mutants ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", P.SMALL)
def test_comparators_score_single_digits(name, refs):
    """A condition on the METRIC: a backward-stable route scores O(1 .. 10) at cond 1.5e3 and at cond 7e7 alike.  <= 16 is asserted
    for LAPACK in every metric and for the emulation in the per-point ones; its covariance figure is printed (module docstring)."""
    (K, _, _, _, _), _, cmp_ = refs(name)
    print("\n%-16s cond %.1e  %s" % (name, np.linalg.cond(K), "  ".join(
        "%s %s" % (k, "/".join("%.2f" % cmp_[k][r] for r in P.ROUTES)) for k in ("v", "m", "M", "c", "I"))))
    for k in ("v", "m", "M", "c", "I"):
        assert cmp_[k]["lapack"] <= 16.0, (k, cmp_[k])
        if k != "c":
            assert cmp_[k]["b128"] <= 16.0, (k, cmp_[k])


@pytest.mark.parametrize("mutant", sorted(P.MUTANTS))
@pytest.mark.parametrize("name", P.SMALL)
def test_every_mutant_is_rejected_with_a_factor_of_ten(name, mutant, refs):
    (K, B, kd, kzz, al), ref, cmp_ = refs(name)
    c = P.case(name)
    got = P.route_values("lapack", K, B, kd, c["y"], al, None, mutant=mutant, nugget=c["nugget"])
    om = P.omegas(got, ref)
    for k in P.MUTANTS[mutant]:
        bound = P.MARGIN * max(cmp_[k].values())
        print("\n%-16s %-12s omega_%s %.2e   bound %.1f" % (name, mutant, k, om[k], bound))
        assert om[k] >= 10.0 * bound, (name, mutant, k, om[k], bound)


def test_the_max_norm_metric_lets_the_scaled_fill_through(refs):
    """The gap being closed.  `rel = max|a - b| / max|b| <= 1e-10`, the assertion of the older posterior tests, passes the 3e-13 scaling
    of B (2700 ulp on every entry of the cross matrix) on the well-conditioned case, in the variance and in the mean; omega rejects it
    on every case.  The structural mutants are printed: on these point sets (300 points in the cube: every variance small, every row
    needed by some point) the max-norm metric rejects them too, and nothing is claimed for them."""
    passes = {}
    for name in P.SMALL:
        (K, B, kd, kzz, al), ref, cmp_ = refs(name)
        c = P.case(name)
        for mutant in P.REL_BLIND:
            got = P.route_values("lapack", K, B, kd, c["y"], al, None, mutant=mutant, nugget=c["nugget"])
            rv, rm = P.rel(got["v"], ref["val"]["v"]), P.rel(got["m"], ref["val"]["m"])
            print("%-16s %-10s rel(var) %.1e  rel(mean) %.1e  omega_v %.1e" % (name, mutant, rv, rm, P.omegas(got, ref)["v"]))
            passes.setdefault(mutant, []).append(rv <= 1e-10 and rm <= 1e-10)
    assert any(passes["scale-B"]), passes


def test_assembly_bound_restates_the_decimal_one():
    """posterior_ref.assembly_bound, vectorised in float64, against kernel_reference.Reference.bound on sampled pairs, both forms."""
    rng = np.random.default_rng(3)
    for name in P.FROM_POINTS:
        c = P.case(name)
        I, J = rng.integers(0, c["n"], 40), rng.integers(0, P.M_EVAL, 40)
        I[:4], J[:4] = [0, 127, 128, c["n"] - 1], [0, 1, 2, 3]           # coincident pairs: x = 0, T = 0
        R = KR.Reference(c["spec"], c["X"], c["Z"], pairs=(I, J))
        kt = DR.cov_ld(c["spec"], c["X"], c["Z"])
        assert np.max(np.abs(np.asarray(kt, dtype=float)[I, J] - R.kf)) <= 4 * P.U * np.max(R.kf)
        for form, cen in (("diff", None), ("expanded", np.array([0.05, -0.02, 0.01]))):
            mine = P.assembly_bound(c["spec"], c["X"], c["Z"], kt, form, cen)[I, J]
            theirs = np.array([float(v) for v in R.bound(form, cen)])
            assert np.max(np.abs(mine / theirs - 1.0)) <= 1e-12, (name, form)


def test_from_points_reference_and_its_allowance(refs):
    """From the points the comparators (on the true arrays rounded once to float64) score what they score on given arrays, and the
    assembly's allowance is tens of u S: the from-points rule is the looser one, the tight rule the one that sees the solve."""
    name = "se-tiny-noise"
    c = P.case(name)
    al = P.host_alpha(name)
    ref = P.reference_from_points(c["spec"], c["X"], c["Z"], c["nugget"], c["y"], al, want_cov=True)
    f = ref["f64"]
    cmp_ = P.comparator_omegas(ref, f["K"], f["B"], f["kd"], c["y"], al, f["kzz"])
    ratio = ref["allow"]["v"] / (P.U * ref["scale"]["v"])
    print("\nfrom points %s: comparators %s; allowance / (u S_v) %.1f .. %.1f"
          % (name, {k: "%.2f" % max(v.values()) for k, v in cmp_.items()}, ratio.min(), ratio.max()))
    for k in ("v", "m", "M", "I"):
        assert 0.0 < max(cmp_[k].values()) <= 16.0, (k, cmp_[k])
    assert 1.0 <= ratio.min() and ratio.max() <= 200.0
    # the host stand-in of the fill (cov_f64, coordinate differences) lies inside the allowance
    K, B, kd, kzz = P.host_arrays(name)
    got = P.route_values("lapack", K, B, kd, c["y"], al, kzz)
    for k, w in P.omegas(got, ref).items():
        assert w <= P.MARGIN * max(cmp_[k].values()), (k, w)


def test_pairwise_mean_restatement():
    rng = np.random.default_rng(9)
    for m in (1, 2, 3, 130, 1023, 1024, 1025, 2049):
        v = rng.integers(-1000, 1000, m).astype(float)
        assert P.pairwise_mean(v) == v.sum() / m          # integers: every order gives the exact sum
    for m in (3, 130, 1025):                              # and the scalar loop of api.hip, entry by entry
        v = rng.standard_normal(m) * 10.0 ** rng.uniform(-6, 0, m)
        w, k = list(v), m
        while k > 1:
            h = (k + 1) // 2
            for i in range(k - h):
                w[i] += w[i + h]
            k = h
        assert P.pairwise_mean(v) == w[0] / float(m)
