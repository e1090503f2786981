"""Golden data of the spectral-density API from the REFERENCE (f-dangel/curvlinops), CPU, float64.

TEST INFRASTRUCTURE ONLY.  Writes ``tests/golden/spectrum.npz``: dense symmetric test matrices, the start vectors the
reference draws, its ``fast_lanczos`` output, densities of both ``*_from_iter`` functions and of the top-level functions
for given boundaries, and its ``approximate_boundaries*`` results.  Only data is stored, no reference source.

    python -B tools/make_golden_spectrum.py --reference <checkout of curvlinops>

The reference imports two third-party packages that are absent here (``einconv``, ``linear_operator``)
and that the spectrum code never calls: raising stubs for them are written to a temporary directory.
"""

from __future__ import annotations

import argparse
import sys
import tempfile
from pathlib import Path

import numpy as np
import torch
from scipy.sparse.linalg import ArpackNoConvergence

OUT = Path(__file__).resolve().parent.parent / "tests" / "golden" / "spectrum.npz"

STUBS = {
    "einconv/__init__.py": "def index_pattern(*a, **k):\n    raise NotImplementedError\n",
    "einconv/utils.py": "def get_conv_paddings(*a, **k):\n    raise NotImplementedError\n",
    "linear_operator/__init__.py": "",
    "linear_operator/utils/__init__.py": "",
    "linear_operator/utils/linear_cg.py": "def linear_cg(*a, **k):\n    raise NotImplementedError\n",
}

NCV = 40
NUM_POINTS = 256
SEED = {"psd": 11, "indef": 12}


def matrices() -> dict[str, np.ndarray]:
    rng = np.random.default_rng(0)
    out = {}
    # PSD with a decaying spectrum (curvature-like), D = 200
    D = 200
    Q, _ = np.linalg.qr(rng.standard_normal((D, D)))
    lam = 10.0 * np.exp(-np.arange(D) / 40.0)
    out["psd"] = (Q * lam) @ Q.T
    # indefinite, D = 160: a bulk around zero and a few outliers on both sides
    D = 160
    Q, _ = np.linalg.qr(rng.standard_normal((D, D)))
    lam = np.concatenate([rng.uniform(-0.5, 0.8, D - 5), [-3.0, -2.2, 4.0, 6.5, 9.0]])
    out["indef"] = (Q * lam) @ Q.T
    for k in out:
        out[k] = (out[k] + out[k].T) / 2
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of f-dangel/curvlinops")
    args = ap.parse_args()
    stubs = Path(tempfile.mkdtemp())
    for rel, text in STUBS.items():
        (stubs / rel).parent.mkdir(parents=True, exist_ok=True)
        (stubs / rel).write_text(text)
    sys.dont_write_bytecode = True
    sys.path[:0] = [str(stubs), args.reference]

    from curvlinops.examples import TensorLinearOperator
    from curvlinops.papyan2020traces import spectrum as S

    torch.set_default_dtype(torch.float64)
    rec: dict[str, np.ndarray] = {"meta/ncv": np.array(NCV), "meta/num_points": np.array(NUM_POINTS)}
    for name, M in matrices().items():
        A = TensorLinearOperator(torch.as_tensor(M))
        lam = np.linalg.eigvalsh(M)
        rec[f"{name}/matrix"] = M
        rec[f"{name}/eigvals"] = lam
        seed = SEED[name]
        torch.manual_seed(seed)
        rec[f"{name}/start"] = torch.randn(M.shape[0]).numpy()
        torch.manual_seed(seed)
        evals, evecs = S.fast_lanczos(A, NCV)
        rec[f"{name}/evals"] = evals.numpy()
        rec[f"{name}/weights"] = (evecs[0] ** 2).numpy()
        bounds = (float(lam[0]), float(lam[-1]))
        abs_bounds = (float(np.abs(lam).min()), float(np.abs(lam).max()))
        rec[f"{name}/bounds"] = np.array(bounds)
        rec[f"{name}/abs_bounds"] = np.array(abs_bounds)
        g, d = S.lanczos_approximate_spectrum_from_iter((evals, evecs), bounds, NUM_POINTS, 3.0, 0.05)
        rec[f"{name}/iter_grid"], rec[f"{name}/iter_density"] = g.numpy(), d.numpy()
        g, d = S.lanczos_approximate_log_spectrum_from_iter((evals, evecs), abs_bounds, NUM_POINTS, 1.04, 0.05, 1e-5)
        rec[f"{name}/iter_log_grid"], rec[f"{name}/iter_log_density"] = g.numpy(), d.numpy()
        # top-level functions, three repeats (running average over successive randn starts)
        torch.manual_seed(seed)
        g, d = S.lanczos_approximate_spectrum(A, NCV, num_points=NUM_POINTS, num_repeats=3, boundaries=bounds)
        rec[f"{name}/spec_grid"], rec[f"{name}/spec_density"] = g.numpy(), d.numpy()
        torch.manual_seed(seed)
        g, d = S.lanczos_approximate_log_spectrum(A, NCV, num_points=NUM_POINTS, num_repeats=3, boundaries=abs_bounds)
        rec[f"{name}/log_grid"], rec[f"{name}/log_density"] = g.numpy(), d.numpy()
        rec[f"{name}/approx_bounds"] = np.array(S.approximate_boundaries(A, tol=1e-8), dtype=np.float64)
        # ARPACK's "SM" mode (no shift-invert) does not converge on an indefinite bulk around zero: record what converges
        try:
            rec[f"{name}/approx_abs_bounds"] = np.array(S.approximate_boundaries_abs(A, tol=1e-2), dtype=np.float64)
        except ArpackNoConvergence:
            print(f"{name}: approximate_boundaries_abs did not converge, not recorded")
    OUT.parent.mkdir(exist_ok=True)
    np.savez_compressed(OUT, **rec)
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
