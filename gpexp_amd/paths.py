"""Base draws of pathwise posterior sampling (gpx_paths_*), made on the host: the device makes no random numbers and never needs
to know a kernel's spectral density.

A stationary kernel k(r) = signalSize * kappa(r) is the Fourier transform of a probability density p(omega) (Bochner), so with
omega_j ~ p and phase_j uniform in [0, 2 pi) the features phi_j(z) = sqrt(2 signalSize / L) cos(omega_j . z + phase_j) satisfy
E[sum_j phi_j(z) phi_j(z')] = k(z, z').  The frequencies come from UNIT draws g ~ N(0, I) (and u ~ chi^2(2 nu) for a Matern
kernel), scaled by the hyper-parameters:

    squared exponential   omega_j[l] = g_j[l] / cl_l                         (p = N(0, diag(1 / cl^2)))
    Matern nu             omega_j    = g_j / rho * sqrt(2 nu / u_j)          (p = multivariate t with 2 nu degrees of freedom)

The Matern line is the spectral density of THIS project's parameterisation, t = sqrt(2 nu) r / rho (gpx.h: sqrt(3) / rho and
sqrt(5) / rho): k is then the standard Matern with length scale rho, whose spectral density is a multivariate t of 2 nu degrees of
freedom and scale 1 / rho, i.e. a normal vector divided by sqrt(u / (2 nu)).
"""
import numpy as np

from . import device as _dev

TWO_NU = {_dev.K_MATERN32: 3, _dev.K_MATERN52: 5}


def spectralFrequencies(spec, g, u=None):
    """omega (L, d) of a device KernelSpec from the unit draws g (L, d) [and u (L,), chi^2(2 nu), for a Matern kernel]."""
    g = np.asarray(g, dtype=np.float64)
    if spec.kind == _dev.K_SE:
        return np.ascontiguousarray(g / spec.hyp[:spec.d][None, :])
    if spec.kind in TWO_NU:
        if u is None:
            raise ValueError("a Matern kernel needs the chi-square draws u of the PathBase (drawn for kernel=None or another kind?)")
        return np.ascontiguousarray(g / spec.hyp[0] * np.sqrt(TWO_NU[spec.kind] / np.asarray(u, dtype=np.float64))[:, None])
    raise NotImplementedError("pathwise sampling needs a stationary kernel (squared exponential, Matern 3/2, Matern 5/2): the "
                              "Mehler kernel has no spectral density")


class PathBase(object):
    """The base draws of S paths with L features on N training points in d dimensions:
        g (L, d) standard normal;  u (L,) chi^2(2 nu) or None (squared exponential);  phase (L,) uniform in [0, 2 pi);
        w (S, L) standard normal;  xi (S, N) standard normal -- the noise draw is eps = sqrt(noise) xi.
    The same PathBase gives the same paths, bit for bit.
    On a VFE model (GP.vfePathSampler) the update lives in the inducing space and takes TWO draws per inducing point: the base is
    drawn with nTrain = 2 nu, xi[:, :nu] is Xi1 (the nugget draw of the inducing variables, eps_u = sqrt(noise) Xi1) and xi[:, nu:]
    is Xi2 (the draw of the variational distribution q(u))."""

    def __init__(self, g, u, phase, w, xi):
        self.g = np.ascontiguousarray(g, dtype=np.float64)
        self.u = None if u is None else np.ascontiguousarray(u, dtype=np.float64)
        self.phase = np.ascontiguousarray(phase, dtype=np.float64)
        self.w = np.ascontiguousarray(w, dtype=np.float64)
        self.xi = np.ascontiguousarray(xi, dtype=np.float64)
        L = self.g.shape[0]
        if self.g.ndim != 2 or L < 1 or self.phase.shape != (L,) or (self.u is not None and self.u.shape != (L,)):
            raise ValueError("PathBase: g is (L >= 1, d), phase (L,), u (L,) or None")
        if self.w.ndim != 2 or self.w.shape[0] < 1 or self.w.shape[1] != L or self.xi.ndim != 2 or self.xi.shape[0] != self.w.shape[0]:
            raise ValueError("PathBase: w is (S >= 1, L) and xi (S, N)")
        for a in (self.g, self.u, self.phase, self.w, self.xi):
            if a is not None and not np.all(np.isfinite(a)):
                raise ValueError("PathBase: the base draws must be finite")
        if self.u is not None and not np.all(self.u > 0.0):
            raise ValueError("PathBase: the chi-square draws u must be positive")

    nPaths = property(lambda self: self.w.shape[0])
    nFeatures = property(lambda self: self.g.shape[0])
    nTrain = property(lambda self: self.xi.shape[1])
    dimension = property(lambda self: self.g.shape[1])

    @classmethod
    def draw(cls, nPaths, nFeatures, nTrain, d, kernel, rng=None):
        """Draw one with NumPy.  `kernel`: a kernel object, a device KernelSpec or a kind id -- it only decides whether u is drawn
        (chi^2 with 3 / 5 degrees of freedom for Matern 3/2 / 5/2).  `rng`: a numpy Generator, a seed, or None (fresh entropy)."""
        S, L, N, d = int(nPaths), int(nFeatures), int(nTrain), int(d)
        if S < 1 or L < 1 or N < 0 or d < 1:
            raise ValueError("PathBase.draw: needs nPaths >= 1, nFeatures >= 1, nTrain >= 0, d >= 1")
        spec = kernel._spec() if hasattr(kernel, "_spec") else kernel
        kind = int(getattr(spec, "kind", spec))
        if kind != _dev.K_SE and kind not in TWO_NU:
            raise NotImplementedError("pathwise sampling needs a stationary kernel (squared exponential, Matern 3/2, Matern 5/2)")
        rng = rng if isinstance(rng, np.random.Generator) else np.random.default_rng(rng)
        g = rng.standard_normal((L, d))
        u = rng.chisquare(TWO_NU[kind], L) if kind in TWO_NU else None
        phase = rng.uniform(0.0, 2.0 * np.pi, L)
        w = rng.standard_normal((S, L))
        xi = rng.standard_normal((S, N))
        return cls(g, u, phase, w, xi)

    def rows(self, sel):
        """The PathBase of the paths `sel` (an index array or slice) alone: same features, those rows of w and xi."""
        return PathBase(self.g, self.u, self.phase, np.atleast_2d(self.w[sel]), np.atleast_2d(self.xi[sel]))
