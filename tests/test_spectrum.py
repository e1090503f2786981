"""Spectral-density API (Papyan 2020; curvlinops_amd/spectrum.py) on CPU: public names and signatures, boundary
estimates with partially given boundaries, float64 parity with the reference's goldens (tests/golden/spectrum.npz,
tools/make_golden_spectrum.py), block chains, and the chain cache."""

import inspect
from math import isclose

import numpy as np
import pytest
import torch

import curvlinops_amd as C
from curvlinops_amd import spectrum as S
from conftest import load_golden

NAMES = ["lanczos_approximate_spectrum", "lanczos_approximate_log_spectrum", "LanczosApproximateSpectrumCached",
         "LanczosApproximateLogSpectrumCached"]


class Dense(C.PyTorchLinearOperator):
    """Explicit symmetric matrix as an operator; counts the products and the columns it was applied to.  Columns are
    multiplied one by one, so a block product rounds exactly like the single-vector products of the reference (without
    reorthogonalisation, Lanczos on an indefinite bulk amplifies rounding differences to ~1e-6 in 40 steps)."""

    SELF_ADJOINT = True

    def __init__(self, M):
        super().__init__([(M.shape[1],)], [(M.shape[0],)])
        self.M = M
        self.columns = 0
        self.products = 0

    def _matmat(self, X):
        self.products += 1
        self.columns += X[0].shape[1]
        return [torch.stack([self.M @ x for x in X[0].unbind(-1)], dim=-1)]

    device = property(lambda self: self.M.device)
    dtype = property(lambda self: self.M.dtype)


def _cluster_weights(evals, weights, rel=1e-6):
    """Weights summed over clusters of (numerically) equal nodes: without reorthogonalisation Lanczos produces ghost
    copies of converged Ritz values, and how eigh splits a weight between two equal nodes is arbitrary (the density, a
    function of nodes and weights, is not affected)."""
    evals, weights = np.asarray(evals), np.asarray(weights)
    cut = np.flatnonzero(np.diff(evals) > rel * np.abs(evals).max()) + 1
    return np.array([w.sum() for w in np.split(weights, cut)]), len(cut)


def _defaults(fn):
    return {k: p.default for k, p in inspect.signature(fn).parameters.items() if p.default is not inspect.Parameter.empty}


def test_public_names_and_signatures():
    for name in NAMES:
        assert name in C.__all__ and getattr(C, name) is getattr(S, name)
    common = {"num_points": 1024, "num_repeats": 1, "boundaries": None, "margin": 0.05, "boundaries_tol": 1e-2}
    assert _defaults(S.lanczos_approximate_spectrum) == {**common, "kappa": 3.0}
    assert _defaults(S.lanczos_approximate_log_spectrum) == {**common, "kappa": 1.04, "epsilon": 1e-5}
    assert list(inspect.signature(S.lanczos_approximate_spectrum).parameters)[:2] == ["A", "ncv"]
    assert _defaults(S.LanczosApproximateSpectrumCached.__init__) == {"boundaries": None, "boundaries_tol": 1e-2}
    assert _defaults(S.LanczosApproximateLogSpectrumCached.__init__) == {"boundaries": None, "boundaries_tol": 1e-2}
    assert _defaults(S.LanczosApproximateSpectrumCached.approximate_spectrum) == {
        "num_repeats": 1, "num_points": 1024, "kappa": 3.0, "margin": 0.05}
    assert _defaults(S.LanczosApproximateLogSpectrumCached.approximate_log_spectrum) == {
        "num_repeats": 1, "num_points": 1024, "kappa": 3.0, "margin": 0.05, "epsilon": 1e-5}
    sig = inspect.signature(S.fast_lanczos).parameters
    assert list(sig)[:3] == ["A", "ncv", "use_eigh_tridiagonal"] and sig["use_eigh_tridiagonal"].default is False
    assert sig["start"].kind is inspect.Parameter.KEYWORD_ONLY and sig["start"].default is None
    for fn in (S.approximate_boundaries, S.approximate_boundaries_abs):
        assert _defaults(fn) == {"tol": 1e-2, "boundaries": None}
    for fn in ("lanczos_approximate_spectrum_from_iter", "lanczos_approximate_log_spectrum_from_iter"):
        assert callable(getattr(S, fn))


@pytest.mark.parametrize("absolute", [False, True])
def test_approximate_boundaries_partial(absolute):
    """The reference's two boundary tests: diag(1..5) and diag(-2, -1, 3, 4, 5), every partial-boundary case."""
    diag = torch.tensor([-2.0, -1.0, 3.0, 4.0, 5.0] if absolute else [1.0, 2.0, 3.0, 4.0, 5.0]).double()
    A = Dense(diag.diag())
    vals = diag.abs() if absolute else diag
    lo, hi = vals.min().item(), vals.max().item()
    fn = S.approximate_boundaries_abs if absolute else S.approximate_boundaries
    cases = [((0.0, 10.0), (0.0, 10.0)), ((1.5, None), (1.5, hi)), ((None, 2.5), (lo, 2.5)), ((None, None), (lo, hi)),
             (None, (lo, hi))]
    for given, want in cases:
        out = fn(A, boundaries=given)
        assert len(out) == 2 and all(type(x) is float for x in out)
        assert isclose(out[0], want[0]) and isclose(out[1], want[1]), (given, out, want)


@pytest.mark.parametrize("case", ["psd", "indef"])
def test_fast_lanczos_matches_reference_goldens(case):
    rec = load_golden("spectrum")[case]
    ncv = int(load_golden("spectrum")["meta"]["ncv"])
    A = Dense(torch.as_tensor(rec["matrix"]))
    start = torch.as_tensor(rec["start"])
    for tridiagonal in (False, True):
        evals, evecs = S.fast_lanczos(A, ncv, tridiagonal, start=start)
        assert evals.dtype == torch.float64 and evecs.shape == (ncv, ncv)
        np.testing.assert_allclose(evals.numpy(), rec["evals"], rtol=0, atol=1e-10 * np.abs(rec["evals"]).max())
        got, n_got = _cluster_weights(evals.numpy(), (evecs[0] ** 2).numpy())
        want, n_want = _cluster_weights(rec["evals"], rec["weights"])
        assert n_got == n_want
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-10)
    evals, evecs = S.fast_lanczos(A, ncv, start=start)
    n = rec["iter_density"]
    g, d = S.lanczos_approximate_spectrum_from_iter((evals, evecs), tuple(rec["bounds"]), len(n), 3.0, 0.05)
    np.testing.assert_allclose(g.numpy(), rec["iter_grid"], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(d.numpy(), n, rtol=0, atol=1e-10 * n.max())
    n = rec["iter_log_density"]
    g, d = S.lanczos_approximate_log_spectrum_from_iter((evals, evecs), tuple(rec["abs_bounds"]), len(n), 1.04, 0.05, 1e-5)
    np.testing.assert_allclose(g.numpy(), rec["iter_log_grid"], rtol=1e-12)
    np.testing.assert_allclose(d.numpy(), n, rtol=0, atol=1e-10 * n.max())


@pytest.mark.parametrize("case", ["psd", "indef"])
def test_density_functions_match_reference_goldens(case):
    """Three repeats from the global generator (the reference's start vectors, drawn in order): the chains run as one
    block here, the densities are the reference's running averages."""
    rec = load_golden("spectrum")[case]
    meta = load_golden("spectrum")["meta"]
    ncv, npts = int(meta["ncv"]), int(meta["num_points"])
    seed = {"psd": 11, "indef": 12}[case]
    A = Dense(torch.as_tensor(rec["matrix"]))
    torch.manual_seed(seed)
    g, d = C.lanczos_approximate_spectrum(A, ncv, num_points=npts, num_repeats=3, boundaries=tuple(rec["bounds"]))
    np.testing.assert_allclose(g.numpy(), rec["spec_grid"], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(d.numpy(), rec["spec_density"], rtol=0, atol=1e-10 * rec["spec_density"].max())
    assert A.products == ncv   # the three chains shared every operator product
    torch.manual_seed(seed)
    g, d = C.lanczos_approximate_log_spectrum(A, ncv, num_points=npts, num_repeats=3,
                                              boundaries=tuple(rec["abs_bounds"]))
    np.testing.assert_allclose(g.numpy(), rec["log_grid"], rtol=1e-12)
    np.testing.assert_allclose(d.numpy(), rec["log_density"], rtol=0, atol=1e-10 * rec["log_density"].max())


@pytest.mark.parametrize("case", ["psd", "indef"])
def test_boundaries_match_reference(case):
    rec = load_golden("spectrum")[case]
    A = Dense(torch.as_tensor(rec["matrix"]))
    lo, hi = S.approximate_boundaries(A, tol=1e-8)
    np.testing.assert_allclose([lo, hi], rec["approx_bounds"], rtol=1e-7)
    np.testing.assert_allclose([lo, hi], rec["bounds"], rtol=1e-7)
    if "approx_abs_bounds" in rec:   # (ARPACK "SM" at tol 1e-2: a loose estimate, as the reference's)
        lo, hi = S.approximate_boundaries_abs(A)
        np.testing.assert_allclose([lo, hi], rec["approx_abs_bounds"], rtol=1e-2)


def test_block_start_equals_single_chains():
    rec = load_golden("spectrum")["psd"]
    A = Dense(torch.as_tensor(rec["matrix"]))
    gen = torch.Generator().manual_seed(3)
    start = torch.randn(A.shape[1], 5, generator=gen, dtype=torch.float64)
    pairs = S.fast_lanczos(A, 25, start=start)
    assert isinstance(pairs, list) and len(pairs) == 5
    for r, (evals, evecs) in enumerate(pairs):
        e1, v1 = S.fast_lanczos(A, 25, start=start[:, r])
        np.testing.assert_allclose(evals.numpy(), e1.numpy(), rtol=0, atol=1e-10)
        np.testing.assert_allclose(_cluster_weights(evals.numpy(), (evecs[0] ** 2).numpy())[0],
                                   _cluster_weights(e1.numpy(), (v1[0] ** 2).numpy())[0], rtol=0, atol=1e-10)
    with pytest.raises(ValueError):
        S.fast_lanczos(A, 5, start=torch.randn(A.shape[1] + 1, dtype=torch.float64))


def test_default_start_draws_like_reference():
    """Without ``start``, one ``randn(D)`` from the global generator (the reference's draw)."""
    rec = load_golden("spectrum")["psd"]
    A = Dense(torch.as_tensor(rec["matrix"]))
    torch.manual_seed(11)
    evals, _ = S.fast_lanczos(A, 12)
    e1, _ = S.fast_lanczos(A, 12, start=torch.as_tensor(rec["start"]))
    np.testing.assert_allclose(evals.numpy(), e1.numpy(), rtol=0, atol=1e-12)


@pytest.mark.parametrize("log", [False, True])
def test_cached_classes_compute_only_missing_chains(log):
    rec = load_golden("spectrum")["psd"]
    A = Dense(torch.as_tensor(rec["matrix"]))
    ncv = 15
    cls = S.LanczosApproximateLogSpectrumCached if log else S.LanczosApproximateSpectrumCached
    cached = cls(A, ncv, boundaries=tuple(rec["abs_bounds" if log else "bounds"]))
    run = cached.approximate_log_spectrum if log else cached.approximate_spectrum
    assert A.columns == 0   # given boundaries: no estimation
    torch.manual_seed(0)
    g2, d2 = run(num_repeats=2, num_points=64)
    assert A.columns == 2 * ncv and A.products == ncv   # two chains, one block
    run(num_repeats=2, num_points=32, kappa=2.0)
    assert A.columns == 2 * ncv                         # cached
    run(num_repeats=5, num_points=64)
    assert A.columns == 5 * ncv and A.products == 2 * ncv   # only the 3 new chains, one more block
    # same numbers as the uncached function from the same generator state
    fn = C.lanczos_approximate_log_spectrum if log else C.lanczos_approximate_spectrum
    torch.manual_seed(0)
    kw = {"kappa": 3.0} if log else {}
    g, d = fn(A, ncv, num_points=64, num_repeats=2, boundaries=tuple(rec["abs_bounds" if log else "bounds"]), **kw)
    np.testing.assert_allclose(d2.numpy(), d.numpy(), rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(g2.numpy(), g.numpy(), rtol=1e-12)


def test_chain_block_rule():
    assert S.chain_block(1000) == 32
    assert S.chain_block(10_010_122) == 32
    assert S.chain_block(100_000_000) == 5
    assert S.chain_block(10**12) == 1
