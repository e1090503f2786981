"""Top-k eigensolver benchmark at C2 (MLP 1024-2688-2688-10, D = 10 010 122, MSE, one batch of 8): prints one JSON line.

- ``eigsh`` with the defaults (block products, block 8): k = 1, 10, 32 for ``LA`` on the GGN and k = 10 for ``LM`` on the
  Hessian -- wall time, operator columns used (counted by wrapping the operator's products).
- The SciPy route ``scipy.sparse.linalg.eigsh(A.to_scipy())`` on the same operators and tolerance (``--skip-scipy``).
- The basis kernels alone at m in {64, 256}, b = 8: time per call and algorithmic bytes over time as a fraction of the
  6.29 TB/s copy rate (kernel-only figures come from a ``rocprofv3 --kernel-trace --stats`` run of ``--kernels-only``,
  tabulated by ``--trace <kernel_trace.csv>``).
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch
from scipy.sparse.linalg import eigsh as scipy_eigsh
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import curvlinops_amd as C  # noqa: E402
from curvlinops_amd import _hip  # noqa: E402

COPY_RATE = 6.29e12


def counting(op):
    """Wraps ``op.__matmul__`` to count the columns it is applied to."""
    count = {"columns": 0}
    orig = op.__matmul__

    class Counted(type(op)):
        def __matmul__(self, X):
            count["columns"] += 1 if X.dim() == 1 else X.shape[1]
            return orig(X)

    op.__class__ = Counted
    return count


def kernels(dev, D, repeats):
    out = {}
    gen = torch.Generator(device=dev).manual_seed(0)
    b = 8
    for m in (64, 256):
        Q = torch.randn(D, m, device=dev, generator=gen)
        W = torch.randn(D, b, device=dev, generator=gen)
        ws = _hip.basis_ws(D, m, b, dev)
        Cc = _hip.basis_project(Q, W, ws) / D
        S = torch.randn(m, b, device=dev, dtype=torch.float64, generator=gen)
        calls = {
            "project": (lambda: _hip.basis_project(Q, W, ws), 4 * D * (m + b)),
            "update": (lambda: _hip.basis_update(W, Q, Cc), 4 * D * (m + 2 * b)),
            "update_reproject": (lambda: _hip.basis_update(W, Q, Cc, ws, reproject=True), 4 * D * (m + 2 * b)),
            "combine": (lambda: _hip.basis_combine(Q, S), 4 * D * (m + b)),
        }
        for name, (fn, nbytes) in calls.items():
            fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(repeats):
                fn()
            torch.cuda.synchronize()
            t = (time.perf_counter() - t0) / repeats
            out[f"{name}_m{m}_b{b}"] = {"ms": round(t * 1e3, 4), "bytes": nbytes,
                                        "copy_rate_fraction": round(nbytes / t / COPY_RATE, 3)}
        del Q, W, ws
        torch.cuda.empty_cache()
    return out


def trace_table(path: str, D: int = 10010122, b: int = 8) -> str:
    """Per-call kernel times of a ``--kernels-only`` run from rocprofv3's ``*_kernel_trace.csv``: medians in call order
    (per m: project x 6 (one more call makes the update's coefficients), update x 6, update + reproject x 6, combine x 6;
    the update kernel is ``<1>`` at m = 64 and ``<4>`` at m = 256), with the algorithmic bytes over kernel time."""
    import csv
    import statistics

    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    ks = [(r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3, r["Grid_Size_Y"])
          for r in rows if "basis_" in r["Kernel_Name"]]
    lines = []
    for m, tag in ((64, "<1>"), (256, "<4>")):
        proj = [t for n, t, g in ks if "project_kernel" in n and g == str(-(-m // 64))]
        upd = [t for n, t, _ in ks if "update_kernel" + tag in n]
        parts = (("project", proj, 4 * D * (m + b)), ("update", upd[0:6], 4 * D * (m + 2 * b)),
                 ("update+reproject", upd[6:12], 4 * D * (m + 2 * b)), ("combine", upd[12:18], 4 * D * (m + b)))
        for name, ts, nbytes in parts:
            t = statistics.median(ts)
            lines.append(f"{name:18s} m={m:4d} b={b}  kernel {t:8.1f} us  {nbytes / 1e9:6.2f} GB  "
                         f"{nbytes / (t * 1e-6) / 1e12:5.2f} TB/s  {nbytes / (t * 1e-6) / COPY_RATE:5.2f} of 6.29 TB/s")
    red = [t for n, t, _ in ks if "reduce" in n]
    lines.append(f"basis_reduce_kernel median {statistics.median(red):.1f} us over {len(red)} launches")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-scipy", action="store_true")
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--tol", type=float, default=1e-4)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--trace", help="print the per-call table of a --kernels-only rocprofv3 kernel trace (CSV) and exit")
    args = ap.parse_args()
    if args.trace:
        print(trace_table(args.trace))
        return
    dev = torch.device("cuda:0")
    _hip.load()
    torch.manual_seed(0)
    model = nn.Sequential(nn.Linear(1024, 2688), nn.ReLU(), nn.Linear(2688, 2688), nn.ReLU(), nn.Linear(2688, 10)).to(dev)
    X, y = torch.rand(8, 1024, device=dev), torch.rand(8, 10, device=dev)
    params = dict(model.named_parameters())
    D = sum(p.numel() for p in params.values())
    res = {"config": "C2", "D": D, "tol": args.tol}
    res["kernels"] = kernels(dev, D, args.repeats)
    if args.kernels_only:
        print(json.dumps(res))
        return
    ops = {"ggn": C.GGNLinearOperator(model, nn.MSELoss(), params, [(X, y)], check_deterministic=False),
           "hessian": C.HessianLinearOperator(model, nn.MSELoss(), params, [(X, y)], check_deterministic=False)}
    runs = [("ggn", 1, "LA"), ("ggn", 10, "LA"), ("ggn", 32, "LA"), ("hessian", 10, "LM")]
    res["eigsh"] = {}
    for name, k, which in runs:
        op = ops[name]
        count = counting(op)
        C.eigsh(op, k=k, which=which, tol=args.tol)   # warm-up
        torch.cuda.synchronize()
        count["columns"] = 0
        t0 = time.perf_counter()
        w = C.eigsh(op, k=k, which=which, tol=args.tol, return_eigenvectors=False)
        torch.cuda.synchronize()
        t = time.perf_counter() - t0
        entry = {"device_s": round(t, 4), "device_columns": count["columns"], "top": float(w[-1])}
        if not args.skip_scipy:
            count["columns"] = 0
            t0 = time.perf_counter()
            ws = scipy_eigsh(op.to_scipy(), k=k, which=which, tol=args.tol, return_eigenvectors=False)
            t_sp = time.perf_counter() - t0
            entry.update({"scipy_s": round(t_sp, 4), "scipy_columns": count["columns"],
                          "speedup": round(t_sp / t, 1), "scipy_top": float(max(ws))})
        res["eigsh"][f"{name}_{which}_k{k}"] = entry
    print(json.dumps(res))


if __name__ == "__main__":
    main()
