"""Spectral-density benchmark at C2 (MLP 1024-2688-2688-10, D = 10 010 122, GGN, MSE, one batch of 8): prints one
JSON line with

- the fused recurrence step ``clo_lanczos_step_f32`` alone: us per step and its 28 D K bytes as a fraction of the
  6.29 TB/s copy rate, K = 1 and K = 32, next to the unfused torch restatement of the reference's step;
- ``lanczos_approximate_spectrum(ncv=128)`` with given boundaries at num_repeats = 1 and 8, next to the reference's loop
  restated in torch (one chain after the other, eight elementwise / reduction launches per step) over the same operator;
- the boundary estimate of the largest eigenvalue (``boundaries=(0, None)``): device solver vs SciPy ``eigsh`` over
  ``to_scipy()`` (the lower end of this rank-80 GGN is the null space, which neither route resolves quickly).

    python benchmarks/bench_spectrum.py [--batch 8] [--skip-host]
"""

import argparse, json, os, sys, time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from torch import nn

import curvlinops_amd as C
from curvlinops_amd import _hip
from curvlinops_amd import spectrum as S

COPY_RATE = 6.29e12


def timed(fn, repeats=3):
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best


def reference_loop(A, ncv, num_repeats, boundaries):
    """The reference's ``lanczos_approximate_spectrum`` restated in torch: chains one after the other, the tridiagonal
    matrices decomposed on the host (as the package does; torch eigh on ROCm is avoided)."""
    out = []
    for _ in range(num_repeats):
        dim = A.shape[1]
        alphas = torch.zeros(ncv, device=A.device)
        betas = torch.zeros(ncv - 1, device=A.device)
        v = torch.randn(dim, device=A.device)
        v /= torch.linalg.vector_norm(v)
        v_prev = None
        for m in range(ncv):
            v_next = A @ v if m == 0 else A @ v - betas[m - 1] * v_prev
            alphas[m] = (v_next * v).sum()
            v_next -= alphas[m] * v
            if m < ncv - 1:
                betas[m] = torch.linalg.vector_norm(v_next)
                v_next /= betas[m]
                v_prev, v = v, v_next
        a, b = alphas.double().cpu().numpy(), betas.double().cpu().numpy()
        import numpy as np

        evals, evecs = np.linalg.eigh(np.diag(a) + np.diag(b, 1) + np.diag(b, -1))
        out.append(S.lanczos_approximate_spectrum_from_iter(
            (torch.as_tensor(evals, device=A.device), torch.as_tensor(evecs, device=A.device)), boundaries, 1024, 3.0,
            0.05))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--skip-host", action="store_true", help="skip the host eigsh boundary route")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = nn.Sequential(nn.Linear(1024, 2688), nn.ReLU(), nn.Linear(2688, 2688), nn.ReLU(), nn.Linear(2688, 10)).to(dev)
    X, y = torch.rand(args.batch, 1024, device=dev), torch.rand(args.batch, 10, device=dev)
    G = C.GGNLinearOperator(model, nn.MSELoss(), dict(model.named_parameters()), [(X, y)], check_deterministic=False)
    D = G.shape[1]
    res = {"config": "C2", "D": D, "batch": args.batch}

    # ---- the recurrence step alone
    f64 = dict(device=dev, dtype=torch.float64)
    for K in (1, 32):
        W, U, P = (torch.randn(D, K, device=dev) for _ in range(3))
        sc, sp, bp = torch.ones(K, **f64), torch.ones(K, **f64), torch.full((K,), 0.5, **f64)
        al, be, sn = (torch.empty(K, **f64) for _ in range(3))
        ws = _hip.lanczos_ws(D, K, dev)
        n = 50

        def fused():
            for _ in range(n):
                _hip.lanczos_step(W, U, P, sc, sp, bp, al, be, sn, ws, first=False, last=False)

        t = timed(fused) / n
        res[f"step_fused_us_k{K}"] = round(t * 1e6, 2)
        res[f"step_fused_bytes_k{K}"] = 28 * D * K
        res[f"step_fused_frac_copy_k{K}"] = round(28 * D * K / t / COPY_RATE, 3)
        if K == 1:
            w0, v, vp = W[:, 0].clone(), U[:, 0].clone(), P[:, 0].clone()
            a, b = torch.zeros(1, device=dev), torch.full((1,), 0.5, device=dev)

            def unfused():
                for _ in range(n):
                    vn = w0 - b[0] * vp
                    a[0] = (vn * v).sum()
                    vn -= a[0] * v
                    b[0] = torch.linalg.vector_norm(vn)
                    vn /= b[0]

            t = timed(unfused) / n
            res["step_unfused_torch_us_k1"] = round(t * 1e6, 2)
        del W, U, P, ws
        torch.cuda.empty_cache()

    # ---- whole densities, boundaries given
    bounds = (0.0, S.approximate_boundaries(G, boundaries=(0.0, None))[1])
    for R in (1, 8):
        res[f"spectrum_ncv128_r{R}_ms"] = round(
            timed(lambda: C.lanczos_approximate_spectrum(G, 128, num_repeats=R, boundaries=bounds), repeats=2) * 1e3, 1)
        res[f"spectrum_ncv128_r{R}_reference_loop_ms"] = round(
            timed(lambda: reference_loop(G, 128, R, bounds), repeats=2) * 1e3, 1)

    # ---- boundaries
    res["boundary_la_device_ms"] = round(timed(lambda: S.approximate_boundaries(G, boundaries=(0.0, None)), 2) * 1e3, 1)
    if not args.skip_host:
        from scipy.sparse.linalg import eigsh

        A_scipy = G.to_scipy()
        t0 = time.perf_counter()
        eigsh(A_scipy, k=1, which="LA", tol=1e-2, return_eigenvectors=False)
        res["boundary_la_host_eigsh_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    res["lambda_max"] = bounds[1]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
