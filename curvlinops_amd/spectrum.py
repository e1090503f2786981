"""Spectral densities of curvature operators (Papyan 2020, https://jmlr.org/papers/v21/20-933.html): Lanczos quadrature
(algorithm 2, ``LanczosApproxSpec``) of ``p(lambda) = 1/d sum_i delta(lambda - lambda_i)`` and of the density of
``log(|A| + eps I)`` (section C.7), with the reference's public API (``curvlinops/papyan2020traces/spectrum.py``).

On fp32 GPU operators:

- ``fast_lanczos`` runs ``R`` chains as the columns of ONE ``[D, R]`` block: one ``A @ V`` per step (the K-column kernels
  of the curvature operators) and one fused recurrence step ``clo_lanczos_step_f32`` (two launches, 28 D R bytes, alpha /
  beta left on the device; the host reads them once, after the loop).  The density functions build missing chains in
  blocks of up to ``chain_block(D)`` columns.
- ``approximate_boundaries*`` run Lanczos with full reorthogonalisation on the device (``[D, 64]`` basis, CGS2 through
  ``clo_tall_gram_f64`` / ``clo_tall_apply_f32``, explicit restarts) instead of ARPACK over ``to_scipy()``.

Every other operator (CPU, float64) takes a plain torch restatement of the same recurrence, and the boundaries use
SciPy's ``eigsh`` over ``to_scipy()`` as the reference does.
"""

from __future__ import annotations

import warnings
from math import log, sqrt

import numpy as np
import torch
from scipy.linalg import eigh_tridiagonal
from scipy.sparse.linalg import eigsh
from torch import Tensor

from curvlinops_amd import _hip
from curvlinops_amd.linop import PyTorchLinearOperator
from curvlinops_amd.trace import project_out

_Boundaries = tuple[float, float] | tuple[float, None] | tuple[None, float] | None

# Chains per block: 32 columns (the K-column kernels' sweet spot), lowered so that the four [D, K] fp32 blocks of the
# recurrence (U, P, A U and the start) stay within 8 GiB: K = min(32, 2^31 / (4 D)) -- 32 up to D = 16.7M (C2: 32).
_MAX_CHAINS = 32
_CHAIN_BYTES = 8 << 30


def chain_block(dim: int) -> int:
    """Largest number of chains ``lanczos_approximate_*`` run as one block for an operator of dimension ``dim``."""
    return max(1, min(_MAX_CHAINS, _CHAIN_BYTES // (16 * max(dim, 1))))


def _native(A: PyTorchLinearOperator) -> bool:
    return A.device.type == "cuda" and A.dtype == torch.float32


# ----------------------------------------------------------------------------------------------------------- densities
def lanczos_approximate_spectrum(
    A: PyTorchLinearOperator,
    ncv: int,
    num_points: int = 1024,
    num_repeats: int = 1,
    kappa: float = 3.0,
    boundaries: _Boundaries = None,
    margin: float = 0.05,
    boundaries_tol: float = 1e-2,
) -> tuple[Tensor, Tensor]:
    """Spectral density ``p(lambda)`` of the symmetric operator ``A`` on a grid of ``num_points`` points, averaged over
    ``num_repeats`` Lanczos quadratures of ``ncv`` nodes (Papyan 2020, algorithm 2).  The spectrum is mapped to [-1, 1]
    (``boundaries``, estimated to ``boundaries_tol`` where not given, widened by ``margin``) and every node becomes a
    Gaussian bump whose width is set by ``kappa > 1``.  Returns ``(grid, density)``."""
    boundaries = approximate_boundaries(A, tol=boundaries_tol, boundaries=boundaries)
    average = torch.zeros(num_points, device=A.device, dtype=A.dtype)
    for n, lanczos_iter in enumerate(_chains(A, ncv, num_repeats)):
        grid, density = lanczos_approximate_spectrum_from_iter(lanczos_iter, boundaries, num_points, kappa, margin)
        average = (1 - 1 / (n + 1)) * average + density / (n + 1)
    return grid, average


def lanczos_approximate_spectrum_from_iter(
    lanczos_iter: tuple[Tensor, Tensor],
    boundaries: tuple[float, float],
    num_points: int,
    kappa: float,
    margin: float,
) -> tuple[Tensor, Tensor]:
    """Density of one Lanczos quadrature ``(evals, evecs)``: nodes ``evals`` with weights ``evecs[0]**2``, each smoothed
    by a Gaussian of width ``sigma = 2 / (ncv - 1) / sqrt(8 log kappa)`` in the normalised coordinates."""
    lo, hi = boundaries
    pad = margin * (hi - lo)
    lo, hi = lo - pad, hi + pad
    c, d = (hi + lo) / 2, (hi - lo) / 2
    evals, evecs = lanczos_iter
    grid_norm = torch.linspace(-1, 1, num_points, device=evals.device, dtype=evals.dtype)
    nodes = (evals - c) / d
    weights = evecs[0, :] ** 2 / d
    density = (weights[:, None] * _gauss(grid_norm[None, :], nodes[:, None], _sigma(evals.shape[0], kappa))).sum(0)
    return torch.linspace(lo, hi, num_points, device=evals.device, dtype=evals.dtype), density


def lanczos_approximate_log_spectrum(
    A: PyTorchLinearOperator,
    ncv: int,
    num_points: int = 1024,
    num_repeats: int = 1,
    kappa: float = 1.04,
    boundaries: _Boundaries = None,
    margin: float = 0.05,
    boundaries_tol: float = 1e-2,
    epsilon: float = 1e-5,
) -> tuple[Tensor, Tensor]:
    """Spectral density of ``log(|A| + epsilon I)`` (natural logarithm; Papyan 2020, section C.7); ``boundaries`` are
    those of ``|A|``.  Other arguments as ``lanczos_approximate_spectrum``.  Returns ``(grid, density)``."""
    boundaries = approximate_boundaries_abs(A, tol=boundaries_tol, boundaries=boundaries)
    average = torch.zeros(num_points, device=A.device, dtype=A.dtype)
    for n, lanczos_iter in enumerate(_chains(A, ncv, num_repeats)):
        grid, density = lanczos_approximate_log_spectrum_from_iter(lanczos_iter, boundaries, num_points, kappa, margin,
                                                                   epsilon)
        average = (1 - 1 / (n + 1)) * average + density / (n + 1)
    return grid, average


def lanczos_approximate_log_spectrum_from_iter(
    lanczos_iter: tuple[Tensor, Tensor],
    boundaries: tuple[float, float],
    num_points: int,
    kappa: float,
    margin: float,
    epsilon: float,
) -> tuple[Tensor, Tensor]:
    """Density of ``log(|A| + epsilon I)`` from one Lanczos quadrature: nodes ``log(|evals| + epsilon)``, weights
    ``evecs[0]**2``, on a grid that is uniform in the logarithm (returned as ``exp`` of it)."""
    lo, hi = (log(b + epsilon) for b in boundaries)
    pad = margin * (hi - lo)
    lo, hi = lo - pad, hi + pad
    c, d = (hi + lo) / 2, (hi - lo) / 2
    evals, evecs = lanczos_iter
    grid_norm = torch.linspace(-1, 1, num_points, device=evals.device, dtype=evals.dtype)
    grid_out = (grid_norm * d + c).exp()
    nodes = ((evals.abs() + epsilon).log() - c) / d
    weights = evecs[0, :] ** 2
    bumps = _gauss(grid_norm[None, :], nodes[:, None], _sigma(evals.shape[0], kappa))
    density = (weights[:, None] * bumps).sum(0) / (d * grid_out)
    return grid_out, density


def _sigma(ncv: int, kappa: float) -> float:
    return 2 / (ncv - 1) / sqrt(8 * log(kappa))


def _gauss(x: Tensor, mu: Tensor, sigma: float) -> Tensor:
    """Normal density ``N(x; mu, sigma^2)`` (as ``exp`` of the log-density, like ``torch.distributions.Normal``)."""
    return (-((x - mu) ** 2) / (2 * sigma**2) - log(sigma) - 0.5 * log(2 * np.pi)).exp()


# ------------------------------------------------------------------------------------------------------ cached classes
class _LanczosSpectrumCached:
    """Keeps the Lanczos quadratures of ``A`` so densities with other hyper-parameters reuse them; asking for more
    repeats computes only the missing chains (in blocks of up to ``chain_block(D)``)."""

    def __init__(self, A: PyTorchLinearOperator, ncv: int):
        self._A = A
        self._ncv = ncv
        self._lanczos_iters: list[tuple[Tensor, Tensor]] = []

    def _get_lanczos_iters(self, num_iters: int) -> list[tuple[Tensor, Tensor]]:
        missing = num_iters - len(self._lanczos_iters)
        if missing > 0:
            self._lanczos_iters.extend(_chains(self._A, self._ncv, missing))
        return self._lanczos_iters[:num_iters]


class LanczosApproximateSpectrumCached(_LanczosSpectrumCached):
    """Spectral density of ``A`` from cached Lanczos quadratures (boundaries estimated once, at construction)."""

    def __init__(self, A: PyTorchLinearOperator, ncv: int, boundaries: _Boundaries = None, boundaries_tol: float = 1e-2):
        super().__init__(A, ncv)
        self._boundaries = approximate_boundaries(A, tol=boundaries_tol, boundaries=boundaries)

    def approximate_spectrum(self, num_repeats: int = 1, num_points: int = 1024, kappa: float = 3.0,
                             margin: float = 0.05) -> tuple[Tensor, Tensor]:
        """``(grid, density)`` averaged over the first ``num_repeats`` cached quadratures."""
        spectra = [lanczos_approximate_spectrum_from_iter(it, self._boundaries, num_points, kappa, margin)
                   for it in self._get_lanczos_iters(num_repeats)]
        return spectra[0][0], sum(s[1] for s in spectra) / num_repeats


class LanczosApproximateLogSpectrumCached(_LanczosSpectrumCached):
    """Spectral density of ``log(|A| + eps I)`` from cached Lanczos quadratures (boundaries of ``|A|`` estimated once)."""

    def __init__(self, A: PyTorchLinearOperator, ncv: int, boundaries: _Boundaries = None, boundaries_tol: float = 1e-2):
        super().__init__(A, ncv)
        self._boundaries = approximate_boundaries_abs(A, tol=boundaries_tol, boundaries=boundaries)

    def approximate_log_spectrum(self, num_repeats: int = 1, num_points: int = 1024, kappa: float = 3.0,
                                 margin: float = 0.05, epsilon: float = 1e-5) -> tuple[Tensor, Tensor]:
        """``(grid, density)`` of ``log(|A| + epsilon I)`` averaged over the first ``num_repeats`` cached quadratures."""
        spectra = [lanczos_approximate_log_spectrum_from_iter(it, self._boundaries, num_points, kappa, margin, epsilon)
                   for it in self._get_lanczos_iters(num_repeats)]
        return spectra[0][0], sum(s[1] for s in spectra) / num_repeats


# ------------------------------------------------------------------------------------------------------------- Lanczos
def _chains(A: PyTorchLinearOperator, ncv: int, num: int) -> list[tuple[Tensor, Tensor]]:
    """``num`` quadratures with the reference's start vectors (one ``randn(D)`` per chain, in order, from torch's global
    generator), run in blocks of ``chain_block(D)`` chains."""
    out: list[tuple[Tensor, Tensor]] = []
    dim, block = A.shape[1], chain_block(A.shape[1])
    while len(out) < num:
        r = min(block, num - len(out))
        if r == 1:
            out.append(fast_lanczos(A, ncv))
            continue
        start = torch.stack([torch.randn(dim, device=A.device, dtype=A.dtype) for _ in range(r)], dim=1)
        out.extend(fast_lanczos(A, ncv, start=start))
    return out


def fast_lanczos(A: PyTorchLinearOperator, ncv: int, use_eigh_tridiagonal: bool = False, *, start: Tensor | None = None):
    """``ncv`` Lanczos steps without reorthogonalisation (Papyan 2020, algorithm 2) and the eigen-decomposition of the
    tridiagonal matrix they build: ``(evals, evecs)`` with ``evecs[:, i]`` the unit eigenvector of ``evals[i]``.

    ``start``: starting vector(s) ``[D]`` or ``[D, R]`` (normalised here); default one ``randn(D)`` on ``A.device``.  A
    ``[D, R]`` start with ``R > 1`` runs the ``R`` chains as one block and returns a list of ``R`` pairs.  The
    tridiagonal matrices are decomposed on the host in float64 (dense ``eigh``, or ``eigh_tridiagonal`` with
    ``use_eigh_tridiagonal=True``); the results are returned on ``A.device`` in ``A.dtype``."""
    device, dtype = A.device, A.dtype
    dim = A.shape[1]
    if start is None:
        start = torch.randn(dim, device=device, dtype=dtype)
    if start.dim() not in (1, 2) or start.shape[0] != dim:
        raise ValueError(f"start must have shape [{dim}] or [{dim}, R], got {tuple(start.shape)}")
    single = start.dim() == 1
    S = start.reshape(dim, -1).to(device=device, dtype=dtype)
    run = _lanczos_native if _native(A) else _lanczos_torch
    alphas, betas = run(A, ncv, S)   # host float64 [ncv, R], [ncv - 1, R]
    pairs = []
    for r in range(S.shape[1]):
        if use_eigh_tridiagonal:
            evals, evecs = eigh_tridiagonal(alphas[:, r], betas[:, r])
        else:
            T = np.diag(alphas[:, r]) + np.diag(betas[:, r], 1) + np.diag(betas[:, r], -1)
            evals, evecs = np.linalg.eigh(T)
        pairs.append((torch.as_tensor(evals, device=device, dtype=dtype),
                      torch.as_tensor(evecs, device=device, dtype=dtype)))
    return pairs[0] if single else pairs


def _lanczos_torch(A: PyTorchLinearOperator, ncv: int, S: Tensor) -> tuple[np.ndarray, np.ndarray]:
    """The reference's recurrence in torch (any device / dtype).  The chains are kept as the contiguous ROWS of an
    ``[R, D]`` array, so every per-chain reduction runs over one contiguous vector, as in the reference's loop."""
    R = S.shape[1]
    alphas = torch.zeros(ncv, R, device=S.device, dtype=S.dtype)
    betas = torch.zeros(max(ncv - 1, 0), R, device=S.device, dtype=S.dtype)
    v = S.T.contiguous()
    v /= torch.linalg.vector_norm(v, dim=1, keepdim=True)
    v_prev = None
    for m in range(ncv):
        w = (A @ v.T).T.contiguous()
        if m:
            w -= betas[m - 1, :, None] * v_prev
        alphas[m] = (w * v).sum(1)
        w -= alphas[m, :, None] * v
        if m < ncv - 1:
            betas[m] = torch.linalg.vector_norm(w, dim=1)
            w /= betas[m, :, None]
            v_prev, v = v, w
    return alphas.double().cpu().numpy(), betas.double().cpu().numpy()


def _lanczos_native(A: PyTorchLinearOperator, ncv: int, S: Tensor) -> tuple[np.ndarray, np.ndarray]:
    """``R`` chains as one ``[D, R]`` block: per step one ``A @ U`` and one ``clo_lanczos_step_f32``; alpha / beta stay
    in ``[ncv, R]`` float64 device arrays and reach the host in one copy after the loop."""
    dim, R = S.shape
    dev = S.device
    U = S.contiguous().clone()   # (the first step's P: the caller's start is never overwritten)
    P = torch.empty_like(U)
    alpha = torch.zeros(ncv, R, device=dev, dtype=torch.float64)
    beta = torch.zeros(ncv, R, device=dev, dtype=torch.float64)
    scales = [1.0 / torch.linalg.vector_norm(U.double(), dim=0), torch.empty(R, device=dev, dtype=torch.float64),
              torch.empty(R, device=dev, dtype=torch.float64)]
    ws = _hip.lanczos_ws(dim, R, dev)
    for m in range(ncv):
        W = (A @ U).contiguous()
        s_cur, s_prev, s_next = scales[m % 3], scales[(m - 1) % 3], scales[(m + 1) % 3]
        _hip.lanczos_step(W, U, P, s_cur, s_prev, beta[m - 1] if m else None, alpha[m], beta[m], s_next, ws,
                          first=m == 0, last=m == ncv - 1)
        U, P = P, U
    host = torch.cat([alpha, beta]).cpu().numpy()   # the one synchronisation of the loop
    return host[:ncv], host[ncv:2 * ncv - 1]


# ---------------------------------------------------------------------------------------------------------- boundaries
def approximate_boundaries(A: PyTorchLinearOperator, tol: float = 1e-2, boundaries: _Boundaries = None
                           ) -> tuple[float, float]:
    """Estimates of ``lambda_min(A)`` and ``lambda_max(A)`` to relative accuracy ``tol`` (``0``: machine precision);
    given entries of ``boundaries`` are kept.  fp32 GPU operators with ``tol > 0`` use the device solver, the rest
    SciPy's ``eigsh`` over ``A.to_scipy()``."""
    lo, hi = (None, None) if boundaries is None else boundaries
    want = {w for w, b in (("SA", lo), ("LA", hi)) if b is None}
    if want and _native(A) and tol > 0:
        found = _device_extremes(A, tol, want)
        if found is not None:
            lo = found["SA"] if lo is None else lo
            hi = found["LA"] if hi is None else hi
            want = set()
    if want:
        kw = {"tol": tol, "return_eigenvectors": False}
        A_scipy = A.to_scipy()
        if want == {"SA", "LA"}:
            lo, hi = eigsh(A_scipy, k=2, which="BE", **kw)
        else:
            if lo is None:
                (lo,) = eigsh(A_scipy, k=1, which="SA", **kw)
            if hi is None:
                (hi,) = eigsh(A_scipy, k=1, which="LA", **kw)
    return float(lo), float(hi)


def approximate_boundaries_abs(A: PyTorchLinearOperator, tol: float = 1e-2, boundaries: _Boundaries = None
                               ) -> tuple[float, float]:
    """Estimates of ``lambda_min(|A|)`` and ``lambda_max(|A|)``; given entries of ``boundaries`` are kept.  On the
    device route the largest magnitude is ``max(|theta_min|, |theta_max|)`` of the converged ends; the smallest is
    ``|theta_min|`` when the spectrum is non-negative (GGN, EF, KFAC), else the smallest-magnitude Ritz value that passes
    the residual test -- and SciPy's ``eigsh(which="SM")`` if none does."""
    lo, hi = (None, None) if boundaries is None else boundaries
    if (lo is None or hi is None) and _native(A) and tol > 0:
        found = _device_extremes(A, tol, {"SA", "LA"})
        if found is not None:
            if hi is None:
                hi = max(abs(found["SA"]), abs(found["LA"]))
            if lo is None:
                if found["SA"] >= -found["floor"]:
                    lo = found["SA"]
                elif found["passing"].size:
                    lo = float(np.abs(found["passing"]).min())
    kw = {"tol": tol, "return_eigenvectors": False}
    if hi is None:
        (hi,) = eigsh(A.to_scipy(), k=1, which="LM", **kw)
    if lo is None:
        (lo,) = eigsh(A.to_scipy(), k=1, which="SM", **kw)
    return abs(float(lo)), abs(float(hi))


_BASIS = 64          # Krylov basis of the device boundary solver ([D, 64]: clo_tall_gram_f64 / clo_tall_apply_f32)
_CHECK_EVERY = 8     # steps between convergence checks (one host synchronisation each)
_MAX_RESTARTS = 8
# float32 operator products resolve eigenvalues only down to ~2^-20 of the largest: the residual test of the ends is
# beta_j |s_ji| <= tol * max(|theta_i|, 2^-20 max|theta|), so an end at (numerically) zero can converge
_FLOOR = 2.0**-20


def _device_extremes(A: PyTorchLinearOperator, tol: float, want: set[str]) -> dict | None:
    """Lanczos with full reorthogonalisation on the device for the wanted ends (``"SA"`` / ``"LA"``).  Returns the
    converged Ritz values of the ends, the Ritz values of the last run that pass the residual test (``"passing"``) and the
    floor of that test, or None (with a ``UserWarning``) when ``_MAX_RESTARTS`` restarts did not converge."""
    dim = A.shape[1]
    dev = A.device
    basis = torch.zeros(dim, _BASIS, device=dev, dtype=torch.float32)
    found: dict = {}
    v0 = torch.randn(dim, 1, device=dev, dtype=torch.float32)
    for _ in range(_MAX_RESTARTS + 1):
        todo = want - found.keys()
        theta, S, resid, ok, m = _reorth_lanczos(A, v0, basis, tol, todo)
        floor = _FLOOR * float(np.abs(theta).max())
        for w in todo:
            i = 0 if w == "SA" else -1
            if ok[i]:
                found[w] = float(theta[i])
        found["floor"] = floor
        found["passing"] = theta[ok]
        if want <= found.keys():
            return found
        # explicit restart from the normalised sum of the unconverged wanted Ritz vectors
        idx = [0 if w == "SA" else m - 1 for w in want - found.keys()]
        coef = torch.zeros(_BASIS, 4, device=dev, dtype=torch.float32)
        coef[:m, 0] = torch.as_tensor(S[:, idx].sum(1), dtype=torch.float32)
        v0 = _hip.tall_apply(basis, coef)[:, :1].contiguous()
    warnings.warn(f"approximate_boundaries: the device Lanczos solver did not converge to tol={tol} within "
                  f"{_MAX_RESTARTS} restarts; falling back to scipy eigsh over to_scipy()", UserWarning, stacklevel=3)
    return None


def _reorth_lanczos(A, v0: Tensor, basis: Tensor, tol: float, todo: set[str]):
    """Up to ``_BASIS`` Lanczos steps from ``v0`` with CGS2 against the basis, checked every ``_CHECK_EVERY`` steps.
    Returns Ritz values, eigenvectors of the tridiagonal matrix, residuals, the residual test and the basis size."""
    dim = A.shape[1]
    dev = A.device
    basis.zero_()
    alpha = torch.zeros(_BASIS, device=dev, dtype=torch.float64)
    beta = torch.zeros(_BASIS, device=dev, dtype=torch.float64)
    scales = [1.0 / torch.linalg.vector_norm(v0.double()).reshape(1), torch.empty(1, device=dev, dtype=torch.float64),
              torch.empty(1, device=dev, dtype=torch.float64)]
    ws = _hip.lanczos_ws(dim, 1, dev)
    U, P = v0.contiguous().clone(), torch.empty(dim, 1, device=dev, dtype=torch.float32)
    result = None
    for j in range(_BASIS):
        s_cur, s_prev, s_next = scales[j % 3], scales[(j - 1) % 3], scales[(j + 1) % 3]
        W = (A @ U).contiguous()
        _hip.lanczos_step(W, U, P, s_cur, s_prev, beta[j - 1: j] if j else None, alpha[j: j + 1], beta[j: j + 1],
                          s_next, ws, first=j == 0, last=False, out=basis[:, j: j + 1])
        Q = basis[:, : -(-(j + 1) // 4) * 4]   # (columns past j are zero: a multiple of 4 avoids a padded copy)
        for _ in range(2):
            P = project_out(Q, P)
        beta[j] = _hip.dot(P, P).double().sqrt()
        torch.reciprocal(beta[j: j + 1], out=s_next)
        U, P = P, U
        if (j + 1) % _CHECK_EVERY == 0 or j == _BASIS - 1:
            result = _ritz(alpha, beta, j + 1, tol, todo)
            if all(result[3][0 if w == "SA" else -1] for w in todo):
                break
    return result


def _ritz(alpha: Tensor, beta: Tensor, m: int, tol: float, todo: set[str]):
    """Ritz values of the leading ``m x m`` tridiagonal matrix (float64, host) and their residuals ``beta_m |s_mi|``.
    A breakdown (non-finite entries after an exhausted Krylov space) truncates to the finite prefix."""
    host = torch.cat([alpha[:m], beta[:m]]).cpu().numpy()
    a, b = host[:m], host[m:]
    bad = ~(np.isfinite(a) & np.isfinite(b))
    if bad.any():
        m = max(int(np.argmax(bad)), 1)
        a, b = a[:m], np.where(np.isfinite(b[:m]), b[:m], 0.0)
    theta, S = np.linalg.eigh(np.diag(a) + np.diag(b[: m - 1], 1) + np.diag(b[: m - 1], -1))
    resid = np.abs(b[m - 1] * S[m - 1, :])
    floor = _FLOOR * float(np.abs(theta).max())
    ok = resid <= tol * np.maximum(np.abs(theta), floor)
    return theta, S, resid, ok, m
