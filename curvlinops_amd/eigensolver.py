"""Top-k eigenpairs of self-adjoint curvature operators on the device: ``eigsh``, a block Lanczos solver with full
reorthogonalisation and thick restart, with the conventions of ``scipy.sparse.linalg.eigsh``.

Per block step of ``b`` columns: one operator product ``A @ Q_j`` (the K-column kernels), CGS2 of the product against the
whole basis (float64 coefficients), and CholQR2 of the result on a float64 Gram matrix, whose small ``b x b`` eigenproblem
is solved on the host.  ``H = Q^T A Q`` is assembled on the host from the coefficients of both passes and the CholQR
factors, symmetrised, and diagonalised in float64 (Rayleigh--Ritz).  When the basis is full, the ``keep`` most wanted
Ritz vectors and the residual block become the start of the next cycle (thick restart, ``keep = k + min(k, (ncv - k) //
2)`` as in ARPACK, at most ``ncv - b``).

On float32 GPU operators the basis passes are HIP kernels (``csrc/basis.hip``): CGS2 is ``clo_basis_project_f64``, then
``clo_basis_update_f32`` with the reprojection fused in, then ``clo_basis_update_f32`` -- three reads of the basis per
block step -- and the Ritz vectors come from ``clo_basis_combine_f32``.  Every other dtype or device runs the same
algorithm with torch ops.
"""

from __future__ import annotations

import numpy as np
import torch
from scipy.sparse.linalg import ArpackNoConvergence
from scipy.sparse.linalg import eigsh as scipy_eigsh
from torch import Tensor

from curvlinops_amd import _hip
from curvlinops_amd.linop import PyTorchLinearOperator

_WHICH = ("LM", "LA", "SA", "BE", "SM")
_DEFAULT_BLOCK = 8
_MAX_NCV = 1024      # widest basis of the basis kernels: ncv + block_size columns (basis and residual block)
_CHECK_EVERY = 4     # block steps between Rayleigh--Ritz checks
_MAX_CYCLES = 200    # default maxiter: basis fills (restart cycles)
# float32 operator products resolve eigenvalues only down to ~2^-20 of the largest (spectrum._FLOOR): a pair converges
# when ||A y - theta y|| <= tol * max(|theta|, 2^-20 max|theta|)
_FLOOR = 2.0**-20
# a direction of a block is DEPENDENT when its singular value after the projections is below this fraction of the
# block's norm before them: float32 products carry ~1e-7 relative rounding noise, so what is left below ~1e-5 is noise
# (an exhausted Krylov space: low-rank GGNs); float64 products resolve down to ~1e-15
_RANK_TOL = {torch.float32: 1e-5, torch.float64: 1e-12}


def eigsh(A: PyTorchLinearOperator, k: int = 6, which: str = "LM", *, ncv: int | None = None,
          block_size: int | None = None, tol: float = 1e-4, maxiter: int | None = None, v0: Tensor | None = None,
          return_eigenvectors: bool = True, generator: torch.Generator | None = None):
    """``k`` eigenpairs of the self-adjoint operator ``A`` (``scipy.sparse.linalg.eigsh`` conventions).

    ``which``: ``"LM"`` / ``"LA"`` / ``"SA"`` / ``"BE"`` (half from each end, the extra one from the top) on the device;
    ``"SM"`` runs SciPy's ``eigsh`` over ``A.to_scipy()``.  Returns ``(w, V)`` -- float64 eigenvalues ``[k]`` in ascending
    order and orthonormal eigenvectors ``[D, k]`` of ``A.dtype``, both on ``A.device`` -- or ``w`` alone with
    ``return_eigenvectors=False``.

    ``ncv``: basis columns (rounded up to a multiple of the block; default ``max(2 k + 2 b, 8 b)``, at most ``1024 - b``
    -- the residual block is held beside the basis); ``block_size``: columns per operator product (default 8); ``tol``: a
    pair has converged when ``||A y - theta y|| <= tol max(|theta|, 2^-20 max|theta|)``, checked with real products before
    returning; pairs whose eigenvalue is zero at the resolution of the dtype (``|theta| <= 64 eps max|theta|``) converge
    once their residual is below that rounding noise instead; ``maxiter``: restart cycles (basis fills) allowed, after
    which ``ArpackNoConvergence`` is raised with the converged pairs; ``v0``: first start column;
    ``generator``: draws the rest of the start block (default: seeded, so repeated calls agree bit for bit)."""
    _check_args(A, k, which)
    if which == "SM":
        # (an explicit start vector: ARPACK's own random start advances a process-wide seed)
        if v0 is None:
            gen = generator if generator is not None else torch.Generator(device=A.device).manual_seed(0)
            v0 = torch.randn(A.shape[0], device=A.device, dtype=torch.float64, generator=gen)
        start = v0.reshape(-1).double().cpu().numpy()
        out = scipy_eigsh(A.to_scipy(), k=k, which="SM", tol=tol, maxiter=maxiter, v0=start,
                          return_eigenvectors=return_eigenvectors)
        if not return_eigenvectors:
            return torch.as_tensor(np.sort(out), device=A.device, dtype=torch.float64)
        w, V = out
        order = np.argsort(w)
        return (torch.as_tensor(w[order], device=A.device, dtype=torch.float64),
                torch.as_tensor(np.ascontiguousarray(V[:, order]), device=A.device, dtype=A.dtype))
    D = A.shape[0]
    b = _DEFAULT_BLOCK if block_size is None else int(block_size)
    if b < 1 or b > 64:
        raise ValueError(f"block_size must be in [1, 64], got {b}")
    maxiter = _MAX_CYCLES if maxiter is None else int(maxiter)
    if D < k + 3 * b:
        w, V = _dense(A, k, which)   # (a Krylov basis with room for the residual block does not fit: decompose densely)
        if maxiter <= 0:
            raise ArpackNoConvergence("eigsh: no restart cycle allowed (maxiter=0)", np.zeros(0), np.zeros((D, 0)))
    else:
        M = -(-(ncv if ncv is not None else max(2 * k + 2 * b, 8 * b)) // b) * b
        M = min(M, (_MAX_NCV - b) // b * b, (D - b) // b * b)
        if M < k + b:
            raise ValueError(f"ncv={ncv} leaves no room: eigsh needs ncv >= k + block_size = {k + b}")
        w, V = _BlockLanczos(A, k, which, M, b, tol, maxiter, v0, generator).run()
    order = torch.argsort(w)
    w, V = w[order], V[:, order]
    return (w, V) if return_eigenvectors else w


def _check_args(A, k: int, which: str) -> None:
    if not isinstance(A, PyTorchLinearOperator):
        raise ValueError(f"eigsh needs a PyTorchLinearOperator, got {type(A).__name__}")
    if A.shape[0] != A.shape[1] or not A.SELF_ADJOINT:
        raise ValueError("eigsh needs a square self-adjoint operator (SELF_ADJOINT = True)")
    if not 1 <= k < A.shape[0]:
        raise ValueError(f"k must satisfy 1 <= k < D = {A.shape[0]}, got {k}")
    if which not in _WHICH:
        raise ValueError(f"which must be one of {_WHICH}, got {which!r}")


def _priority(theta: np.ndarray, which: str) -> np.ndarray:
    """Indices of the Ritz values ``theta`` (ascending) from most to least wanted."""
    n = theta.shape[0]
    if which == "LA":
        return np.arange(n)[::-1]
    if which == "SA":
        return np.arange(n)
    if which == "LM":
        return np.argsort(-np.abs(theta), kind="stable")
    hi, lo, out = n - 1, 0, []   # BE: alternately from the top and the bottom, the top first
    while lo <= hi:
        out.append(hi)
        hi -= 1
        if lo <= hi:
            out.append(lo)
            lo += 1
    return np.asarray(out)


def _dense(A: PyTorchLinearOperator, k: int, which: str) -> tuple[Tensor, Tensor]:
    """Small operators: the dense matrix ``A @ I`` decomposed in float64."""
    D = A.shape[0]
    dense = (A @ torch.eye(D, device=A.device, dtype=A.dtype)).double().cpu().numpy()
    theta, S = np.linalg.eigh((dense + dense.T) / 2)
    idx = _priority(theta, which)[:k]
    return (torch.as_tensor(theta[idx], device=A.device, dtype=torch.float64),
            torch.as_tensor(np.ascontiguousarray(S[:, idx]), device=A.device, dtype=A.dtype))


# ------------------------------------------------------------------------------------------------------- basis ops
class _NativeOps:
    """Basis passes on float32 GPU blocks: the ``csrc/basis.hip`` kernels."""

    def __init__(self, D: int, m: int, b: int, device):
        self.ws = _hip.basis_ws(D, m, b, device)

    def cgs2(self, Q: Tensor, W: Tensor) -> Tensor:
        C1 = _hip.basis_project(Q, W, self.ws)
        C2 = _hip.basis_update(W, Q, C1, self.ws, reproject=True)
        _hip.basis_update(W, Q, C2)
        return C1 + C2

    def gram(self, W: Tensor) -> Tensor:
        return _hip.tall_gram(W)

    def combine(self, Q: Tensor, S: np.ndarray, out: Tensor | None = None) -> Tensor:
        return _hip.basis_combine(Q, torch.as_tensor(S, device=Q.device, dtype=torch.float64).contiguous(), out=out)


class _TorchOps:
    """The same passes in torch (any device / dtype); coefficients and Gram matrices in float64."""

    def cgs2(self, Q: Tensor, W: Tensor) -> Tensor:
        total = None
        for _ in range(2):
            C = Q.double().T @ W.double()
            W -= (Q.double() @ C).to(W.dtype)
            total = C if total is None else total + C
        return total

    def gram(self, W: Tensor) -> Tensor:
        Wd = W.double()
        return Wd.T @ Wd

    def combine(self, Q: Tensor, S: np.ndarray, out: Tensor | None = None) -> Tensor:
        Y = (Q.double() @ torch.as_tensor(S, device=Q.device, dtype=torch.float64)).to(Q.dtype)
        if out is None:
            return Y
        out.copy_(Y)
        return out


# ------------------------------------------------------------------------------------------------------- solver
class _BlockLanczos:
    def __init__(self, A, k, which, M, b, tol, maxiter, v0, generator):
        self.A, self.k, self.which, self.M, self.b, self.tol, self.maxiter = A, k, which, M, b, tol, maxiter
        D, dev, dtype = A.shape[0], A.device, A.dtype
        self.D, self.dev, self.dtype = D, dev, dtype
        self.native = dev.type == "cuda" and dtype == torch.float32
        self.rank_tol = _RANK_TOL.get(dtype, 1e-5)
        if dev.type == "cuda":
            need = 2 * D * (M + b) * dtype.itemsize + 4 * D * b * dtype.itemsize
            free = torch.cuda.mem_get_info(dev)[0]
            if need > free:
                fit = (free // (2 * D * dtype.itemsize) - 3 * b) // b * b
                raise MemoryError(f"eigsh: a basis of ncv={M} columns (+{b}) needs {need / 2**30:.1f} GiB, "
                                  f"{free / 2**30:.1f} GiB free; use ncv <= {max(fit, 0)}")
        self.ops = _NativeOps(D, M + b, b, dev) if self.native else _TorchOps()
        self.Q = torch.zeros(D, M + b, device=dev, dtype=dtype)
        self.Qalt = torch.zeros(D, M + b, device=dev, dtype=dtype)
        if generator is None:
            generator = torch.Generator(device=dev).manual_seed(0)
        self.gen = generator
        X = torch.randn(D, b, device=dev, dtype=dtype, generator=generator)
        if v0 is not None:
            X[:, 0] = v0.reshape(-1).to(device=dev, dtype=dtype)
        self.X0 = X
        self.anorm = 0.0

    # ---- CholQR2 with replacement of dependent directions
    def _orthonormalize(self, W: Tensor, m: int, ref: float, G: np.ndarray | None = None
                        ) -> tuple[np.ndarray, np.ndarray]:
        """Writes an orthonormal basis of ``W`` [D, b] (projected off ``Q[:, :m]``) into ``Q[:, m:m+b]``; returns
        ``(R, extra)`` with ``W = Q[:, m:m+b] R + Q[:, :m] extra``.  Directions of ``W`` below ``rank_tol * ref`` are
        replaced by random directions orthogonal to the basis (their rows of ``R`` are zero).  ``G``: ``W^T W`` if the
        caller has already read it back."""
        b = W.shape[1]
        out = self.Q[:, m: m + b]
        if G is None:
            G = self.ops.gram(W).cpu().numpy()
        lam, V = np.linalg.eigh((G + G.T) / 2)
        keep = lam > (self.rank_tol * ref) ** 2
        r = int(keep.sum())
        R = np.zeros((b, b))
        extra = np.zeros((m, b))
        if r:
            lk, Vk = lam[keep][::-1], V[:, keep][:, ::-1]
            Y = self.ops.combine(W, Vk / np.sqrt(lk))                  # first pass: [D, r]
            if m and lk.min() < (1e-3 * ref) ** 2:
                # the projections cancelled most of the block: what is left carries basis components of the order of the
                # rounding error over its own size, which the normalisation has magnified -- project them out once more
                E = self.ops.cgs2(self.Q[:, :m], Y).cpu().numpy()
                extra = E @ (np.sqrt(lk)[:, None] * Vk.T)   # (W = (Y + Q E) Rk)
            Rk = np.sqrt(lk)[:, None] * Vk.T                            # W (kept part) = Y Rk
            # further passes until the block that goes in is well conditioned (two for any block whose singular values
            # span less than ~1e8; the first pass leaves |Y^T Y - I| ~ eps cond(W)^2)
            for _ in range(3):
                G2 = self.ops.gram(Y).cpu().numpy()
                lam2, V2 = np.linalg.eigh((G2 + G2.T) / 2)
                lam2 = np.maximum(lam2, np.finfo(np.float64).tiny)
                Y = self.ops.combine(Y, V2 / np.sqrt(lam2))
                Rk = (np.sqrt(lam2)[:, None] * V2.T) @ Rk
                if lam2.min() > 0.5 * lam2.max():
                    break
            out[:, :r] = Y
            R[:r] = Rk
        if r < b:
            Z = torch.randn(self.D, b - r, device=self.dev, dtype=self.dtype, generator=self.gen)
            nz = float(torch.linalg.vector_norm(Z.double(), dim=0).max())
            if m + r:
                self.ops.cgs2(self.Q[:, : m + r], Z)
            self._orthonormalize(Z, m + r, nz)
        return R, extra

    def _step(self, m: int) -> tuple[np.ndarray, np.ndarray]:
        """Block step on ``Q[:, m:m+b]``: returns the coefficient column block ``Q[:, :m+b]^T A Q_j`` and ``R``."""
        b = self.b
        W = (self.A @ self.Q[:, m: m + b]).contiguous()
        # directions are judged against the largest product seen so far: a block in (or near) the null space of a
        # low-rank operator has a product made of rounding noise, which must not become a basis direction
        norms = torch.linalg.vector_norm(W, dim=0, dtype=torch.float64)
        coef = self.ops.cgs2(self.Q[:, : m + b], W)
        # the product's norms, the coefficients and the Gram matrix of the projected block in ONE read-back
        host = torch.cat([norms[None, :], coef, self.ops.gram(W)]).cpu().numpy()
        self.anorm = max(self.anorm, float(host[0].max()), 1e-300)
        coef, G = host[1: m + b + 1], host[m + b + 1:]
        R, extra = self._orthonormalize(W, m + b, self.anorm, G)
        return coef + extra, R

    def _ritz(self, H: np.ndarray, m: int, R: np.ndarray):
        Hm = H[:m, :m]
        theta, S = np.linalg.eigh((Hm + Hm.T) / 2)
        resid = np.linalg.norm(R @ S[m - self.b: m, :], axis=0)
        ok = resid <= self._bound(theta, theta)
        return theta, S, ok

    def _bound(self, theta_all: np.ndarray, theta: np.ndarray) -> np.ndarray:
        """Residual bound of the pairs ``theta``: ``tol max(|theta|, 2^-20 max|theta|)``.  Only for eigenvalues that are
        zero at the dtype's resolution (``|theta| <= 64 eps max|theta|``) the bound is raised to that rounding noise: a
        float32 product cannot resolve their residual below it, and the 2^-20 floor alone leaves them unreachable."""
        top = float(np.abs(theta_all).max())
        noise = 64 * torch.finfo(self.dtype).eps * top
        bound = self.tol * np.maximum(np.abs(theta), _FLOOR * top)
        return np.where(np.abs(theta) <= noise, np.maximum(bound, noise), bound)

    def _true_residuals(self, Y: Tensor, theta: np.ndarray) -> np.ndarray:
        AY = self.A @ Y
        th = torch.as_tensor(theta, device=self.dev, dtype=self.dtype)
        return torch.linalg.vector_norm((AY - Y * th).double(), dim=0).cpu().numpy()

    def run(self) -> tuple[Tensor, Tensor]:
        k, b, M = self.k, self.b, self.M
        H = np.zeros((M + b, M + b))
        ref = float(torch.linalg.vector_norm(self.X0.double(), dim=0).max())
        self.Q.zero_()
        self._orthonormalize(self.X0.contiguous(), 0, ref)
        m, cycle, steps = 0, 0, 0
        best = None
        while cycle < self.maxiter:
            R = None
            while m + b <= M:
                coef, R = self._step(m)
                H[: m + b, m: m + b] = coef
                H[m + b: m + 2 * b, m: m + b] = R
                m += b
                steps += 1
                if steps % _CHECK_EVERY and m + b <= M:
                    continue
                theta, S, ok = self._ritz(H, m, R)
                idx = _priority(theta, self.which)[:k]
                best = (theta, S, ok, idx, m)
                if ok[idx].all():
                    Y = self.ops.combine(self.Q[:, :m], S[:, idx])
                    true = self._true_residuals(Y, theta[idx])
                    if np.all(true <= self._bound(theta, theta[idx])):
                        return torch.as_tensor(theta[idx], device=self.dev, dtype=torch.float64), Y
            # ---- thick restart: the most wanted Ritz vectors and the residual block
            cycle += 1
            if cycle >= self.maxiter:
                break
            theta, S, ok, _, _ = best
            keep = min(k + min(k, (M - k) // 2), M - b)
            kidx = _priority(theta, self.which)[:keep]
            self.ops.combine(self.Q[:, :m], S[:, kidx], out=self.Qalt[:, :keep])
            self.Qalt[:, keep: keep + b] = self.Q[:, m: m + b]
            Hn = np.zeros_like(H)
            Hn[np.arange(keep), np.arange(keep)] = theta[kidx]
            Hn[keep: keep + b, :keep] = R @ S[m - b: m, kidx]
            H = Hn
            self.Q, self.Qalt = self.Qalt, self.Q
            m = keep
        return self._no_convergence(best)

    def _no_convergence(self, best):
        if best is None:
            raise ArpackNoConvergence("eigsh: no restart cycle allowed (maxiter=0)", np.zeros(0),
                                      np.zeros((self.D, 0)))
        theta, S, ok, idx, m = best
        conv = idx[ok[idx]]
        w = theta[conv]
        V = self.ops.combine(self.Q[:, :m], S[:, conv]).cpu().numpy() if conv.size else np.zeros((self.D, 0))
        raise ArpackNoConvergence(f"eigsh: {conv.size} of {self.k} eigenpairs converged to tol={self.tol} within "
                                  f"maxiter={self.maxiter} restart cycles", w, V)
