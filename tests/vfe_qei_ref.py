"""Cases, restatements and a NumPy stand-in for Monte-Carlo q-EI on VFE models (gpx_vfe_acq_qei; NumPy only; data and references of
tests/test_vfe_qei_host.py and tests/test_gpu_vfe_qei.py, not product code).  Built on sample_ref (the q-EI replay and its bound, the
factor contract), vfe_sample_ref (the model and its exact covariance in either precision), fitc_grad_ref (the cases) and
chol_stability_ref (u).

The kernel forms, per lower-triangle entry (i, j) of a batch,
    su = sum_r Wu[r][i] Wu[r][j]      sa = sum_r Wa[r][i] Wa[r][j]      (r < nu)         C_b[i][j] = (k(z_i, z_j) - su) + sa
each sum split into nsl slices (row r in slice r mod nsl; nsl from the plan of q), a slice one chain in ascending r, the slices added in
slice order.  `signed_gram` restates that order in float64 (products rounded where the kernel fuses them: the order, not the bits).
Mutants: "signs" (+su - sa), "wa_twice" (Wa read for both factors).
"""
import numpy as np

import chol_stability_ref as CR
import fitc_grad_ref as FR
import sample_ref as SR
import vfe_sample_ref as VS

LD, U = CR.LD, CR.U
TOL = 1e-8                     # the project's figure for VFE quantities against the reference
MUTANTS = ("signs", "wa_twice")

# (kind, d, lengths, signalSize, N, nu, noise, seed) as fitc_grad_ref.case takes them: the seven small cases of
# tests/test_gpu_vfe_sample.py (SMALL + LOW_NOISE), the out-of-place size, and a Mehler model (lengths: its t)
SMALL = [("se", 1, [0.1], 1.0, 5, 1, 1e-2, 31),
         ("matern32", 2, [0.5], 1.4, 9, 3, 1e-2, 32),
         ("matern52", 3, [0.7], 1.1, 40, 17, 1e-2, 33),
         ("se", 8, [1.0, 1.2, 0.8, 1.5, 0.9, 1.1, 1.3, 0.7], 1.0, 130, 40, 1e-2, 34),
         ("matern32", 2, [0.5], 1.4, 257, 129, 1e-2, 35),
         ("matern52", 32, [4.0], 1.2, 40, 16, 1e-2, 36),
         ("matern52", 3, [0.7], 1.1, 40, 17, 1e-6, 37)]
OOP = ("matern52", 8, [1.5], 1.2, 2304, 2049, 0.05, 19)
MEHLER = ("mehler", 2, [0.3, 0.5], None, 40, 16, 1e-2, 41)
QS, BS, SAMPLES = (1, 2, 5, 16, 32), (1, 3, 257), (1, 3, 128, 130)


def case_id(c):
    return "%s-d%d-N%d-nu%d-noise%g" % (c[0], c[1], c[4], c[5], c[6])


def build(c):
    """(spec, X, S, y, noise) of a case; a Mehler model takes the points and values fitc_grad_ref.case makes, drawn into 0.8 x the cube."""
    if c[0] != "mehler":
        return FR.case(c)
    _, X, S, y, noise = FR.case(("se", c[1], [1.0], 1.0) + tuple(c[4:]))
    return dict(kind="mehler", d=c[1], t=list(c[2])), 0.8 * X, 0.8 * S, y, noise


def setting(q, b):
    """(case, S) of the grid point (q, B): the eight cases dealt over the grid, the 257-batch points over those with nu <= 40."""
    i = QS.index(q) * len(BS) + BS.index(b)
    cases = SMALL + [MEHLER]
    if b == 257:
        cases = [c for c in cases if c[5] <= 40]
        return cases[(i // len(BS)) % len(cases)], SAMPLES[i % 4]
    return cases[i % len(cases)], SAMPLES[i % 4]


def batches(c, S, q, nb, seed=0):
    """(nb q, d) uniform in the cube; batch 0 has its second point ON S[0] and, for q >= 5, its last point repeats its first."""
    Zb = np.random.default_rng(100 * q + nb + seed + c[7]).uniform(-1.0, 1.0, (nb * q, c[1]))
    if q >= 2:
        Zb[1] = S[0]
    if q >= 5:
        Zb[q - 1] = Zb[0]
    return Zb


def default_nugget(spec, Zb):
    return 1e-10 * SR.prior_max(spec, Zb)


# ---- the kernel's plan and its Gram order --------------------------------------------------------------------------------------------
def plan(q):
    """(G, T, nsl, npair): batches per workgroup, threads per batch, row slices per entry, entries of the lower triangle."""
    G, npair, T, nsl = 32 // q, q * (q + 1) // 2, 1, 1
    while 2 * T * G <= 256:
        T *= 2
    while 2 * nsl * G * npair <= 256:
        nsl *= 2
    return G, T, nsl, npair


def sliced_gram(W, nsl):
    """W^T W (q, q) of one batch's columns W (nu, q) in float64: row r in slice r mod nsl, a slice accumulated in ascending r, the
    slices added in slice order."""
    W = np.asarray(W, dtype=float)
    total = None
    for sl in range(nsl):
        acc = np.zeros((W.shape[1], W.shape[1]))
        for r in range(sl, W.shape[0], nsl):
            acc = acc + W[r][:, None] * W[r][None, :]
        total = acc if total is None else total + acc
    return total


def signed_gram(kzz, Wu, Wa, q, mutant=None):
    """(k - su) + sa of one batch in the kernel's order (float64)."""
    nsl = plan(q)[2]
    if mutant == "wa_twice":
        Wu = Wa
    su, sa = sliced_gram(Wu, nsl), sliced_gram(Wa, nsl)
    return (kzz + su) - sa if mutant == "signs" else (kzz - su) + sa


def solved(spec, S, m, Zb, dtype=float):
    """(Wu, Wa) = (Lu^-1 K(S, Zb), La^-1 K(S, Zb)) for all batch points at once."""
    Ku = VS.cov(spec, S, Zb, dtype)
    return VS.fwd(m["Lu"], Ku, dtype), VS.fwd(m["La"], Ku, dtype)


def blocks_f64(spec, S, m64, Zb, q, mutant=None):
    """(B, q, q): every batch's covariance by the float64 restatement of the kernel's route."""
    Wu, Wa = solved(spec, S, m64, Zb, float)
    nb = Zb.shape[0] // q
    return np.array([signed_gram(VS.cov(spec, Zb[b * q:(b + 1) * q], None, float), Wu[:, b * q:(b + 1) * q], Wa[:, b * q:(b + 1) * q], q,
                                 mutant) for b in range(nb)])


def blocks_ref(spec, S, m, Zb, q, dtype=LD):
    """(B, q, q): the diagonal q x q blocks of vfe_sample_ref.exact_cov at all batch points, without the blocks between batches."""
    Wu, Wa = solved(spec, S, m, Zb, dtype)
    nb = Zb.shape[0] // q
    out = np.empty((nb, q, q), dtype=dtype)
    for b in range(nb):
        sl = slice(b * q, (b + 1) * q)
        out[b] = VS.cov(spec, Zb[sl], None, dtype) - np.dot(Wu[:, sl].T, Wu[:, sl]) + np.dot(Wa[:, sl].T, Wa[:, sl])
    return out


def worst_rel(got, ref):
    """max over the batches of max |got_b - ref_b| / max |ref| (one scale for the call: max |cov|)."""
    ref = np.asarray(ref)
    return float(np.max(np.abs(np.asarray(got) - ref)) / np.max(np.abs(ref)))


def route_bound(nu, kd):
    """(q, q) bound on the distance between two float64 routes to C_b from bit-identical Wu, Wa and k: each rounds a sum of nu
    products once per term, then two more operations, so it lies within (nu + 2) u (|k_ij| + sqrt(su_ii su_jj) + sqrt(sa_ii sa_jj)) of
    the exact value for the same W; sa_ii <= su_ii <= k_ii (A >= Quu >= Kuu), and two routes take twice that: 6 (nu + 2) u sqrt(k_ii k_jj)."""
    kd = np.asarray(kd, dtype=float)
    return 6.0 * (nu + 2) * U * np.sqrt(kd[:, None] * kd[None, :])


def worst_factor_ratio(Fb, Cb, nugget):
    """max over the batches of |F F^T - (C_b + nugget I)| / sample_ref.factor_bound(q); asserts every F_b lower triangular."""
    q, worst = Fb.shape[1], 0.0
    for b in range(Fb.shape[0]):
        assert np.all(np.triu(Fb[b], 1) == 0.0), "batch %d: F_b is not lower triangular" % b
        Chat = Cb[b].copy()
        Chat[np.diag_indices(q)] += nugget
        worst = max(worst, SR.factor_residual(Fb[b], Chat) / SR.factor_bound(q))
    return worst


# ---- the NumPy stand-in for device.VfeModel ---------------------------------------------------------------------------------------------
class VfeStandin(object):
    """device.VfeModel's acq_qei (and what the class API reads beside it) on host arrays in float64: vfe_sample_ref.exact_cov and
    .mean, then sample_ref.qei_replay; a batch that repeats a point with nugget 0 costs NaN, by the definition.  Records its calls."""

    def __init__(self, spec, X, S, y, noise):
        self.spec, self.S, self.noise, self.calls = spec, S, noise, []
        self.m = VS.model(spec, X, S, y, noise, float)

    def posterior_cov(self, Z):
        return VS.exact_cov(self.spec, self.S, self.m, Z, float)

    def acq_qei(self, coeff, Zb, q, xi, fBest, nugget, want_costs=True):
        self.calls.append(("vfe_qei", Zb.shape[0] // q, q, xi.shape, float(fBest), float(nugget)))
        costs, nbad = [], 0
        for b in range(Zb.shape[0] // q):
            Zq = Zb[b * q:(b + 1) * q]
            C = self.posterior_cov(Zq)
            try:
                if nugget == 0.0 and SR.first_repeated_row(Zq):
                    raise np.linalg.LinAlgError("pivot 0")
                F = np.linalg.cholesky(0.5 * (C + C.T) + nugget * np.eye(q))
                costs.append(float(SR.qei_replay(VS.mean(self.spec, self.S, self.m, Zq, float), F, xi, fBest, dtype=np.float64)))
            except np.linalg.LinAlgError:
                costs.append(float("nan"))
                nbad += 1
        costs = np.array(costs)
        ok = np.flatnonzero(~np.isnan(costs))
        best = int(ok[np.argmin(costs[ok])]) if ok.size else -1
        return best, (costs[best] if best >= 0 else float("nan")), (costs if want_costs else None), nbad
