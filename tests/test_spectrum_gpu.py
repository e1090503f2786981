"""Spectral densities on the MI355X: the fused Lanczos step ``clo_lanczos_step_f32`` against a float64 NumPy restatement
(through the C ABI), the golden matrices as fp32 GPU operators, R chains of an MLP GGN in one block on the K-column
kernels, the device boundary solver, and a full-size C2 density."""

import numpy as np
import pytest
import torch
from torch import nn

import curvlinops_amd as C
from conftest import load_golden
from curvlinops_amd import _hip
from curvlinops_amd import spectrum as S
from test_spectrum import Dense

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    _hip.load()
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ kernel vs NumPy
def _np_step(W, U, P, s_cur, s_prev, beta_prev, first):
    """Float64 restatement of one step on the stored (unnormalised) blocks."""
    w = s_cur * W if first else s_cur * W - (beta_prev * s_prev) * P
    alpha = (w * (s_cur * U)).sum(0)
    w = w - alpha * (s_cur * U)
    beta = np.sqrt((w * w).sum(0))
    return alpha, beta, w


@pytest.mark.parametrize("D", [1, 3, 4097, 2**20 + 5])
@pytest.mark.parametrize("K", [1, 3, 4, 32, 64])
def test_lanczos_step_kernel(dev, D, K):
    gen = torch.Generator(device=dev).manual_seed(D * 131 + K)
    W = torch.randn(D, K, device=dev, generator=gen)
    U = torch.randn(D, K, device=dev, generator=gen)
    P0 = torch.randn(D, K, device=dev, generator=gen)
    f64 = dict(device=dev, dtype=torch.float64)
    s_cur = torch.rand(K, **f64) + 0.5
    s_prev = torch.rand(K, **f64) + 0.5
    beta_prev = torch.rand(K, **f64) + 0.1
    ws = _hip.lanczos_ws(D, K, dev)
    Wn, Un, Pn = (t.double().cpu().numpy() for t in (W, U, P0))
    sc, sp, bp = (t.cpu().numpy() for t in (s_cur, s_prev, beta_prev))
    scale = max(np.abs(Wn).max(), 1.0) * 4
    for first, last, copy in [(True, False, False), (False, False, True), (False, True, False), (False, False, False)]:
        outs = []
        for _ in range(2):   # repeat: bit-identical
            P = P0.clone()
            alpha, beta, s_next = (torch.full((K,), float("nan"), **f64) for _ in range(3))
            basis = torch.full((D, K + 5), -7.0, device=dev) if copy else None
            out = basis[:, 2: 2 + K] if copy else None
            _hip.lanczos_step(W, U, P, s_cur, s_prev, None if first else beta_prev, alpha, beta, s_next, ws,
                              first=first, last=last, out=out)
            torch.cuda.synchronize()
            outs.append((alpha.cpu(), beta.cpu(), s_next.cpu(), P.cpu(), None if basis is None else basis.cpu()))
        for a, b in zip(outs[0], outs[1]):
            assert a is None or torch.equal(a, b)
        alpha, beta, s_next, P, basis = outs[0]
        ra, rb, rw = _np_step(Wn, Un, Pn, sc, sp, bp, first)
        np.testing.assert_allclose(alpha.numpy(), ra, rtol=1e-4, atol=1e-5 * scale * np.sqrt(D))
        np.testing.assert_allclose(beta.numpy(), rb, rtol=1e-4)
        np.testing.assert_allclose(s_next.numpy(), 1 / rb, rtol=1e-4)
        if last:
            assert torch.equal(P, P0.cpu())   # the last step writes no next block
        else:
            np.testing.assert_allclose(P.double().numpy(), rw, rtol=0, atol=1e-6 * max(np.abs(rw).max(), scale))
        if copy:
            np.testing.assert_allclose(basis[:, 2: 2 + K].double().numpy(), sc * Un, rtol=1e-6, atol=1e-6)
            assert (basis[:, :2] == -7).all() and (basis[:, 2 + K:] == -7).all()


def test_lanczos_step_validation(dev):
    lib = _hip.load()
    assert lib.clo_lanczos_step_f32(None, None, None, 4, 65, None, None, None, None, None, None, None, 0, 3, None,
                                    None) == -1
    assert b"K = 65" in lib.clo_last_error()
    assert lib.clo_lanczos_step_f32(None, None, None, -1, 4, None, None, None, None, None, None, None, 0, 3, None,
                                    None) == -1
    assert lib.clo_lanczos_ws_bytes(10, 0) == -1


# ------------------------------------------------------------------------------------- golden matrices on the GPU
# Tolerance of the density, integrated absolute difference (mass displaced) against the reference's float64 density:
# the same recurrence in float32 on the CPU (torch, same start) displaces 0.079 (psd, spectrum), 1.6e-4 (psd, log),
# 5.7e-7 (indef, spectrum) and 0.030 (indef, log) -- Lanczos without reorthogonalisation amplifies rounding, most on
# the decaying PSD spectrum and on log-nodes near zero.  The bounds below are 4x those figures (1e-5 for the smallest).
L1_TOL = {("psd", False): 0.32, ("psd", True): 7e-4, ("indef", False): 1e-5, ("indef", True): 0.12}


@pytest.mark.parametrize("case", ["psd", "indef"])
def test_golden_matrices_fp32_gpu(dev, case):
    G = load_golden("spectrum")
    rec, ncv, npts = G[case], int(G["meta"]["ncv"]), int(G["meta"]["num_points"])
    A = Dense(torch.as_tensor(rec["matrix"], dtype=torch.float32, device=dev))
    evals, evecs = S.fast_lanczos(A, ncv, start=torch.as_tensor(rec["start"], dtype=torch.float32, device=dev))
    assert evals.device.type == "cuda" and evals.dtype == torch.float32
    pair = (evals.double().cpu(), evecs.double().cpu())
    for log in (False, True):
        if log:
            g, d = S.lanczos_approximate_log_spectrum_from_iter(pair, tuple(rec["abs_bounds"]), npts, 1.04, 0.05, 1e-5)
            ref = rec["iter_log_density"]
        else:
            g, d = S.lanczos_approximate_spectrum_from_iter(pair, tuple(rec["bounds"]), npts, 3.0, 0.05)
            ref = rec["iter_density"]
        l1 = np.trapezoid(np.abs(d.numpy() - ref), g.numpy())
        assert l1 < L1_TOL[case, log], (case, log, l1)


# ------------------------------------------------------------------------------------------ MLP GGN, R chains
def _mlp(dev, dims, N, seed=0, act=nn.Tanh):
    torch.manual_seed(seed)
    layers = []
    for i in range(len(dims) - 1):
        layers.append(nn.Linear(dims[i], dims[i + 1]))
        if i < len(dims) - 2:
            layers.append(act())
    model = nn.Sequential(*layers).to(dev)
    X, y = torch.rand(N, dims[0], device=dev), torch.rand(N, dims[-1], device=dev)
    return model, [(X, y)]


def test_mlp_ggn_block_chains_native(dev):
    model, data = _mlp(dev, [40, 64, 48, 6], 32)
    params = dict(model.named_parameters())
    G = C.GGNLinearOperator(model, nn.MSELoss(), params, data, check_deterministic=False)
    assert G.uses_native_kernels
    D, R, ncv = G.shape[1], 8, 12
    start = torch.randn(D, R, device=dev)
    before = G.native_column_products
    pairs = S.fast_lanczos(G, ncv, start=start)
    assert G.native_column_products - before >= ncv   # the K-column kernels ran, one block product per step
    model64 = model.double().cpu()
    params64 = dict(model64.named_parameters())
    G64 = C.GGNLinearOperator(model64, nn.MSELoss(), params64, [(X.double().cpu(), y.double().cpu()) for X, y in data],
                              check_deterministic=False)
    # Without reorthogonalisation, float32 loses orthogonality once the outliers converge (~6 steps here) and the interior
    # Ritz values depart from a float64 run's; what the quadrature is built to keep are its moments
    # sum_i w_i theta_i^k = v0^T A^k v0 (k < 2 ncv) and the converged extreme Ritz value.
    for r, (evals, evecs) in enumerate(pairs):
        e64, v64 = S.fast_lanczos(G64, ncv, start=start[:, r].double().cpu())
        e32, w32 = evals.double().cpu(), evecs[0].double().cpu() ** 2
        w64 = v64[0] ** 2
        scale = float(e64.abs().max())
        assert abs(float(e32[-1]) - float(e64[-1])) <= 1e-4 * scale
        for k in range(5):
            m32, m64 = float((w32 * e32**k).sum()), float((w64 * e64**k).sum())
            assert abs(m32 - m64) <= 1e-4 * scale**k, (r, k, m32, m64)


# ------------------------------------------------------------------------------------------ device boundaries
def _dense(op, dev):
    D = op.shape[1]
    cols = [op @ torch.eye(D, device=dev)[:, i: i + 32].contiguous() for i in range(0, D, 32)]
    M = torch.cat(cols, 1).double().cpu().numpy()
    return (M + M.T) / 2


def test_device_boundaries_ggn(dev):
    """rank(GGN) <= N C = 48 < 64: the Krylov space exhausts the range and both ends converge."""
    model, data = _mlp(dev, [32, 64, 8], 6)
    G = C.GGNLinearOperator(model, nn.MSELoss(), dict(model.named_parameters()), data, check_deterministic=False)
    lam = np.linalg.eigvalsh(_dense(G, dev))
    tol = 1e-2
    floor = 2.0**-20 * lam[-1]
    lo, hi = S.approximate_boundaries(G, tol=tol)
    assert type(lo) is float and type(hi) is float
    assert abs(hi - lam[-1]) <= tol * abs(lam[-1])
    assert abs(lo - lam[0]) <= tol * max(abs(lam[0]), floor) + 4 * floor
    lo_abs, hi_abs = S.approximate_boundaries_abs(G, tol=tol)
    assert abs(hi_abs - np.abs(lam).max()) <= tol * np.abs(lam).max()
    assert abs(lo_abs - np.abs(lam).min()) <= 8 * floor
    lo2, hi2 = S.approximate_boundaries(G, tol=tol, boundaries=(None, 123.0))
    assert hi2 == 123.0 and abs(lo2 - lam[0]) <= tol * max(abs(lam[0]), floor) + 4 * floor


def test_device_boundaries_indefinite_hessian(dev):
    model, data = _mlp(dev, [16, 24, 4], 64)
    H = C.HessianLinearOperator(model, nn.MSELoss(), dict(model.named_parameters()), data, check_deterministic=False)
    lam = np.linalg.eigvalsh(_dense(H, dev))
    assert lam[0] < 0 < lam[-1]
    tol = 1e-2
    lo, hi = S.approximate_boundaries(H, tol=tol)
    assert abs(lo - lam[0]) <= tol * abs(lam[0]) and abs(hi - lam[-1]) <= tol * abs(lam[-1])
    lo_abs, hi_abs = S.approximate_boundaries_abs(H, tol=tol)
    big = np.abs(lam).max()
    assert abs(hi_abs - big) <= tol * big
    # the smallest magnitude: a Ritz value whose residual passed, or eigsh; either is within tol of an eigenvalue
    assert np.abs(np.abs(lam) - lo_abs).min() <= tol * max(lo_abs, 2.0**-20 * big) + 4 * 2.0**-20 * big


# ------------------------------------------------------------------------------------------------- full size C2
def test_c2_density_full_size(dev):
    """BASELINE.json configs[1]: MLP 1024-2688-2688-10 (D = 10 010 122), GGN, ncv = 128, R = 8 chains in one block."""
    torch.manual_seed(0)
    model = nn.Sequential(nn.Linear(1024, 2688), nn.ReLU(), nn.Linear(2688, 2688), nn.ReLU(), nn.Linear(2688, 10)).to(dev)
    X, y = torch.rand(8, 1024, device=dev), torch.rand(8, 10, device=dev)
    G = C.GGNLinearOperator(model, nn.MSELoss(), dict(model.named_parameters()), [(X, y)], check_deterministic=False)
    lo, hi = S.approximate_boundaries(G, boundaries=(0.0, None))
    grid, density = C.lanczos_approximate_spectrum(G, 128, num_repeats=8, boundaries=(lo, hi))
    assert torch.isfinite(density).all() and (density >= 0).all()
    mass = np.trapezoid(density.double().cpu().numpy(), grid.double().cpu().numpy())
    assert abs(mass - 1.0) < 1e-2, mass
