"""The trace estimators' tall-skinny algebra (``curvlinops_amd/trace.py``) on sketches WIDER than 64 columns, fp32 on the
MI355X against plain float64: the float64 Gram matrix from 64-column panels of the basis kernels, the rank-revealing
orthonormal basis, the Gram QR of XTrace / XDiag, the projections, and the estimators end to end.  Hutch++ reaches this
width from ``num_matvecs > 192``, XTrace / XDiag from ``num_matvecs > 128``.  Widths straddle the 64-column tall kernels,
the 16-column tiles of the basis kernels and their 1024-column limit; rows straddle the ``m >= 2 n`` gate of the Gram
route (``2 n - 1`` takes ``torch.linalg.qr``) and the 64-row chunks of the kernels."""

import pytest
import torch
from torch import nn

import curvlinops_amd as C
from curvlinops_amd import _hip
from curvlinops_amd import trace as T

pytestmark = pytest.mark.gpu

F64 = torch.float64
WIDTHS = [64, 65, 68, 96, 127, 128, 129, 200, 256, 1024, 1040]   # 64: the one-pass tall Gram (control)
CHUNK = 2**20   # rows per float64 reference product (the 1e7-row case stays a few GB)


@pytest.fixture(scope="module")
def dev():
    _hip.load()
    return torch.device("cuda:0")


def gen(dev, seed):
    return torch.Generator(device=dev).manual_seed(seed)


def ref_gram(A, B=None):
    """``A^T B`` in float64 (torch), summed over row chunks."""
    B = A if B is None else B
    out = torch.zeros(A.shape[1], B.shape[1], device=A.device, dtype=F64)
    for r in range(0, A.shape[0], CHUNK):
        out += A[r:r + CHUNK].double().T @ B[r:r + CHUNK].double()
    return out


def ortho_err(Q):
    return float((ref_gram(Q) - torch.eye(Q.shape[1], device=Q.device, dtype=F64)).abs().max())


def range_err(X, Q):
    """max |X - Q Q^T X| / max |X| in float64: how far ``X`` is from range(Q)."""
    QtX = ref_gram(Q, X)
    worst = 0.0
    for r in range(0, X.shape[0], CHUNK):
        worst = max(worst, float((X[r:r + CHUNK].double() - Q[r:r + CHUNK].double() @ QtX).abs().max()))
    return worst / float(X.abs().max())


def orthonormal_rows(D, r, dev, g):
    """``[D, r]`` with (near-)orthonormal columns: Householder Q for small blocks, ``randn / sqrt(D)`` for D >= 64 r
    (condition number 1 + O(sqrt(r / D)))."""
    if D >= 64 * r:
        return torch.randn(D, r, device=dev, generator=g) / D ** 0.5
    return torch.linalg.qr(torch.randn(D, r, device=dev, dtype=F64, generator=g))[0].float()


def planted(D, n, r, dev, g, top=0.0, bottom=-4.0):
    """``X = B diag(s) C^T`` of rank r, ``s = logspace(top, bottom, r)``, B and C with orthonormal columns (float32)."""
    B = orthonormal_rows(D, r, dev, g) * torch.logspace(top, bottom, r, device=dev)
    Cm = torch.linalg.qr(torch.randn(n, r, device=dev, dtype=F64, generator=g))[0].float()
    return B @ Cm.T


def rows_for(n):
    """Row counts per width: the gate (2 n, exactly where the Gram route starts) and a ragged count."""
    return sorted({2 * n, max(4099, 2 * n + 3)})


# ------------------------------------------------------------------------------------------------ 1. the Gram matrix
@pytest.mark.parametrize("n", WIDTHS)
def test_gram64(dev, n):
    g = gen(dev, n)
    cases = [(D, False) for D in rows_for(n)] + [(4099 if n <= 1024 else 8195, True)]
    if n in (65, 256):
        cases.append((1_000_003, False))
    for D, strided in cases:
        X = torch.randn(D, n + 3, device=dev, generator=g)[:, :n] if strided else torch.randn(D, n, device=dev, generator=g)
        got = T._gram64(X)
        ref = ref_gram(X)
        assert got.dtype == F64 and got.shape == (n, n)
        err = float((got - ref).abs().max() / ref.abs().max())
        assert err < 1e-12, (n, D, strided, err)
        assert torch.equal(got, got.T), (n, D, strided)


# ----------------------------------------------------------------------------------- 2. the rank-revealing basis
@pytest.mark.parametrize("n", WIDTHS)
def test_orthonormal_basis_planted_rank(dev, n):
    g = gen(dev, 100 + n)
    for D in rows_for(n) + ([1_000_003] if n in (96, 256) else []):
        for r in sorted({40, n // 2, n - 1}):
            X = planted(D, n, r, dev, g)
            Q = T.orthonormal_basis(X, complete=False)
            assert Q.shape == (D, r), (n, D, r, tuple(Q.shape))
            assert ortho_err(Q) < 1e-5, (n, D, r)
            assert range_err(X, Q) < 1e-5, (n, D, r)
            Qc = T.orthonormal_basis(X)
            assert Qc.shape == (D, n)
            assert ortho_err(Qc) < 1e-5 and range_err(X, Qc) < 1e-5, (n, D, r)
        # full rank with an exactly zero and an exactly repeated column
        X = torch.randn(D, n, device=dev, generator=g)
        X[:, 5] = 0.0
        X[:, n - 1] = X[:, 2]
        Q = T.orthonormal_basis(X, complete=False)
        assert Q.shape == (D, n - 2), (n, D, tuple(Q.shape))
        assert ortho_err(Q) < 1e-5 and range_err(X, Q) < 1e-5
        Qc = T.orthonormal_basis(X)
        assert Qc.shape == (D, n) and ortho_err(Qc) < 1e-5 and range_err(X, Qc) < 1e-5


@pytest.mark.parametrize("n", [65, 128, 1040])
def test_orthonormal_basis_below_gate(dev, n):
    """``2 n - 1`` rows: the Householder route, n orthonormal columns whatever ``complete`` says."""
    g = gen(dev, 200 + n)
    X = planted(2 * n - 1, n, n // 2, dev, g)
    Q = T.orthonormal_basis(X, complete=False)
    assert Q.shape == (2 * n - 1, n)
    assert ortho_err(Q) < 1e-5 and range_err(X, Q) < 1e-5


# ------------------------------------------------------------------------------------------ 3. conditioning sweep
@pytest.mark.parametrize("n", [32, 96, 256])
@pytest.mark.parametrize("k", [0, 3, 6, 9, 12])
def test_orthonormal_basis_conditioning(dev, n, k):
    """Singular values ``logspace(0, -k)``: the returned basis is orthonormal whether or not a pass saw a
    well-conditioned input, and spans the directions above the float32 noise floor."""
    g = gen(dev, 300 + 17 * n + k)
    X = planted(20_000, n, n, dev, g, bottom=-float(k))
    for complete in (False, True):
        Q = T.orthonormal_basis(X, complete=complete)
        assert ortho_err(Q) < 1e-5, (n, k, complete, tuple(Q.shape))
        assert range_err(X, Q) < 1e-4, (n, k, complete)
        if complete:
            assert Q.shape == (20_000, n)
        elif k <= 3:
            assert Q.shape == (20_000, n)


# ----------------------------------------------------------------------------------------------- 4. the Gram QR
@pytest.mark.parametrize("n", [65, 128, 129, 256, 1024, 1040])
def test_gram_qr(dev, n):
    g = gen(dev, 400 + n)
    for D in rows_for(n):
        X = torch.randn(D, n, device=dev, generator=g) * torch.logspace(0, -2, n, device=dev)
        qt = T._gram_qr(X)
        assert qt is not None, (n, D)
        Q, RTinv = qt
        assert Q.shape == (D, n) and RTinv.shape == (n, n)
        assert ortho_err(Q) < 1e-5, (n, D)
        Tm = ref_gram(Q, X)                                   # X = Q T
        assert float((Q.double() @ Tm - X.double()).abs().max() / X.abs().max()) < 1e-5, (n, D)
        eye = torch.eye(n, device=dev, dtype=F64)
        err = float((RTinv.double() @ Tm.T - eye).abs().max())
        assert err < 1e-6, (n, D, err)                        # the returned T^-T inverts T^T
        # numerically rank-deficient blocks are refused (XTrace / XDiag then take the float64 QR)
        assert T._gram_qr(planted(D, n, n - 1, dev, g)) is None
        Xz = X.clone()
        Xz[:, 3] = 0.0
        assert T._gram_qr(Xz) is None
        Xd = X.clone()
        Xd[:, n - 1] = Xd[:, 0]
        assert T._gram_qr(Xd) is None


# ------------------------------------------------------------------------------------- 5. / 6. projection, X T
@pytest.mark.parametrize("n", [64, 65, 128, 256, 1024, 1040])
def test_project_out(dev, n):
    g = gen(dev, 500 + n)
    D = 4099 if n <= 1024 else 8195
    Q = T.orthonormal_basis(planted(D, n, n, dev, g, bottom=-2.0))
    assert Q.shape == (D, n)
    for b in (1, 7, 64, 65, 200):
        for strided in (False, True):
            G = torch.randn(D, b + 3, device=dev, generator=g)[:, :b] if strided else torch.randn(D, b, device=dev, generator=g)
            G0 = G.clone()
            got = T.project_out(Q, G)
            assert torch.equal(G, G0), (n, b, strided)         # the caller's block is not modified
            Qd = Q.double()
            ref = G.double() - Qd @ (Qd.T @ G.double())
            err = float((got.double() - ref).abs().max() / G.abs().max())
            assert err < 1e-5, (n, b, strided, err)


@pytest.mark.parametrize("n,p", [(65, 65), (65, 40), (128, 128), (200, 7), (1024, 1024), (1024, 65), (1040, 1040),
                                 (40, 96)])
def test_times_small(dev, n, p):
    g = gen(dev, 600 + n + p)
    D = 4099
    X = torch.randn(D, n, device=dev, generator=g)
    Tm = torch.randn(n, p, device=dev, dtype=F64, generator=g)
    got = T._times_small(X, Tm).double()
    ref = X.double() @ Tm
    scale = X.double().abs() @ Tm.abs()
    assert got.shape == (D, p)
    assert float(((got - ref).abs() / scale).max()) < 1e-5, (n, p)


# --------------------------------------------------------------------------------------------- one C2-size block
def test_wide_block_c2_rows(dev):
    """D = 10 010 122 (the C2 MLP's parameter count), n = 128: the panelled Gram, the rank-revealing basis and the
    Gram QR at the row counts where float32 sums would have lost the small directions."""
    D, n = 10_010_122, 128
    g = gen(dev, 700)
    X = planted(D, n, n - 1, dev, g)
    got = T._gram64(X)
    ref = ref_gram(X)
    assert float((got - ref).abs().max() / ref.abs().max()) < 1e-12 and torch.equal(got, got.T)
    Q = T.orthonormal_basis(X, complete=False)
    assert Q.shape == (D, n - 1)
    assert ortho_err(Q) < 1e-5 and range_err(X, Q) < 1e-5
    assert T._gram_qr(X) is None
    del Q, X
    X = torch.randn(D, n, device=dev, generator=g) * torch.logspace(0, -2, n, device=dev)
    Q, _ = T._gram_qr(X)
    assert ortho_err(Q) < 1e-5
    G = torch.randn(D, 65, device=dev, generator=g)
    P = T.project_out(Q, G)
    assert float(ref_gram(Q, P).abs().max()) < 1e-5 * float(ref_gram(G).diagonal().max()) ** 0.5


# ------------------------------------------------------------------------------------------ 7. / 8. end to end
class LowRank(C.PyTorchLinearOperator):
    """``A = U diag(lam) U^T`` applied in factored form (any dtype / device)."""

    SELF_ADJOINT = True

    def __init__(self, U, lam):
        super().__init__([(U.shape[0],)], [(U.shape[0],)])
        self.U, self.lam = U, lam

    def _matmat(self, X):
        return [self.U @ (self.lam[:, None] * (self.U.T @ X[0]))]

    device = property(lambda self: self.U.device)
    dtype = property(lambda self: self.U.dtype)


def _operators(D, r, lam, dev, seed):
    """The same operator as an fp32 device operator and a float64 CPU operator (U orthonormal in float64)."""
    g = torch.Generator().manual_seed(seed)
    U = torch.linalg.qr(torch.randn(D, r, dtype=F64, generator=g))[0]
    return LowRank(U.float().to(dev), lam.float().to(dev)), LowRank(U, lam), U


def _rel(got, ref):
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    return float(torch.linalg.vector_norm(got - ref) / torch.linalg.vector_norm(ref))


@pytest.mark.parametrize("N", [65, 96, 128, 256])
def test_estimators_decaying_spectrum(dev, N):
    """Rank 3N, ``lam = logspace(0, -6)``: the fp32 device estimators equal float64 torch with the same probes."""
    D = 4099
    lam = torch.logspace(0, -6, 3 * N, dtype=F64)
    A32, A64, _ = _operators(D, 3 * N, lam, dev, N)
    g = torch.Generator().manual_seed(1000 + N)
    for dist in ("rademacher", "normal"):
        S = torch.randn(D, N, dtype=F64, generator=g) if dist == "normal" else \
            torch.randint(0, 2, (D, N), generator=g).double() * 2 - 1
        Gp = torch.randn(D, N, dtype=F64, generator=g)
        S32, G32 = S.float().to(dev), Gp.float().to(dev)
        ref = T.hutchpp_trace(A64, 3 * N, probes=(S, Gp))
        assert _rel(T.hutchpp_trace(A32, 3 * N, probes=(S32, G32)), ref) < 1e-4, (N, dist)
        ref = T.xtrace(A64, 2 * N, probes=S)
        assert _rel(T.xtrace(A32, 2 * N, probes=S32), ref) < 1e-4, (N, dist)
        if dist == "rademacher":
            ref = T.xdiag(A64, 2 * N, probes=S)
            assert _rel(T.xdiag(A32, 2 * N, probes=S32), ref) < 1e-3, N


def test_estimators_decaying_spectrum_large(dev):
    """The same at D = 10^6 (N = 128): float64 reference on the device."""
    D, N = 1_000_003, 128
    g = torch.Generator(device=dev).manual_seed(11)
    U = torch.randn(D, 3 * N, device=dev, dtype=F64, generator=g) / D ** 0.5   # (not orthonormal: any U will do)
    lam = torch.logspace(0, -6, 3 * N, device=dev, dtype=F64)
    A32, A64 = LowRank(U.float(), lam.float()), LowRank(U.float().double(), lam.float().double())
    S = torch.randint(0, 2, (D, N), device=dev, generator=g).double() * 2 - 1
    Gp = torch.randn(D, N, device=dev, dtype=F64, generator=g)
    ref = T.hutchpp_trace(A64, 3 * N, probes=(S, Gp))
    assert _rel(T.hutchpp_trace(A32, 3 * N, probes=(S.float(), Gp.float())), ref) < 1e-4
    ref = T.xtrace(A64, 2 * N, probes=S)
    assert _rel(T.xtrace(A32, 2 * N, probes=S.float()), ref) < 1e-4


@pytest.mark.parametrize("N", [65, 96, 128, 256])
def test_estimators_planted_rank_exact(dev, N):
    """Rank r <= N - 1: the sketch holds the whole range, so Hutch++ and XTrace return the exact trace and XDiag the exact
    diagonal, whatever the probes."""
    D = 4099
    for r in (N - 1, N // 2):
        lam = torch.logspace(0, -3, r, dtype=F64)
        A32, _, U = _operators(D, r, lam, dev, 2000 + N + r)
        exact, diag = float(lam.sum()), (U * U * lam).sum(1)
        g = torch.Generator().manual_seed(r)
        S = torch.randint(0, 2, (D, N), generator=g).float().to(dev) * 2 - 1
        Gp = torch.randint(0, 2, (D, N), generator=g).float().to(dev) * 2 - 1
        assert _rel(T.hutchpp_trace(A32, 3 * N, probes=(S, Gp)), exact) < 1e-5, (N, r)
        assert _rel(T.xtrace(A32, 2 * N, probes=S), exact) < 1e-5, (N, r)
        assert _rel(T.xdiag(A32, 2 * N, probes=S), diag) < 1e-4, (N, r)


# ------------------------------------------------------------------------------------------ 9. a rank-deficient GGN
def test_estimators_rank_deficient_ggn(dev):
    """MLP 20-40-10, CrossEntropyLoss, 8 samples: GGN rank <= 8 * (10 - 1) = 72 < N = 96.  Hutch++ and XTrace on the
    native fp32 operator equal the exact trace ``sum_n tr(J_n^T H_n J_n)`` evaluated in float64 with torch.func."""
    torch.manual_seed(0)
    model = nn.Sequential(nn.Linear(20, 40), nn.Tanh(), nn.Linear(40, 10))
    X, y = torch.randn(8, 20), torch.randint(0, 10, (8,))
    model64 = nn.Sequential(nn.Linear(20, 40), nn.Tanh(), nn.Linear(40, 10)).double()
    model64.load_state_dict({k: v.double() for k, v in model.state_dict().items()})
    params64 = {k: v.detach() for k, v in model64.named_parameters()}

    def f(p, x):
        return torch.func.functional_call(model64, p, (x,))

    J = torch.func.jacrev(f)(params64, X.double())                        # {name: [8, 10, *shape]}
    Jf = torch.cat([J[k].reshape(8, 10, -1) for k in params64], dim=2)    # [8, 10, D], parameter order of the model
    prob = torch.softmax(f(params64, X.double()), dim=1)
    H = (torch.diag_embed(prob) - prob[:, :, None] * prob[:, None, :]) / 8  # mean reduction
    exact = float(torch.einsum("nce,ncd,nde->", Jf, H, Jf))

    model = model.to(dev)
    G = C.GGNLinearOperator(model, nn.CrossEntropyLoss(), dict(model.named_parameters()), [(X.to(dev), y.to(dev))],
                            check_deterministic=False)
    assert G.uses_native_kernels
    D, N = G.shape[1], 96
    g = torch.Generator().manual_seed(5)
    S = (torch.randint(0, 2, (D, N), generator=g).float() * 2 - 1).to(dev)
    Gp = (torch.randint(0, 2, (D, N), generator=g).float() * 2 - 1).to(dev)
    assert _rel(T.hutchpp_trace(G, 3 * N, probes=(S, Gp)), exact) < 1e-4
    assert _rel(T.xtrace(G, 2 * N, probes=S), exact) < 1e-4
    assert T.orthonormal_basis(G @ S, complete=False).shape[1] <= 72


# ---------------------------------------------------------------------------------------- 10. probes at width
@pytest.mark.parametrize("K", [65, 128, 1024])
def test_pack_probes_wide(dev, K):
    D = 100_003
    for dist in ("rademacher", "normal"):
        P = _hip.pack_probes(D, K, 1234 + K, dist, dev)
        assert P.shape == (D, K) and torch.isfinite(P).all()
        if dist == "rademacher":
            assert bool((P.abs() == 1).all())
        Pd = P.double()
        assert float(Pd.mean(0).abs().max()) < 5 / D ** 0.5, (K, dist)
        Pn = Pd / torch.linalg.vector_norm(Pd, dim=0)
        corr = Pn.T @ Pn
        off = corr - torch.diag(corr.diagonal())
        assert float(off.abs().max()) < 6 / D ** 0.5, (K, dist)   # (so no two columns are equal or opposite)
