"""The block eigensolver on the MI355X: the basis kernels of csrc/basis.hip through the C ABI against float64 NumPy,
``eigsh`` on fp32 GPU operators against dense float64 eigendecompositions, a rank-deficient GGN, and the full-size C2
GGN."""

import numpy as np
import pytest
import torch
from torch import nn

import curvlinops_amd as C
from curvlinops_amd import _hip
from curvlinops_amd import spectrum as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    _hip.load()
    return torch.device("cuda:0")


def _strided(D, n, ld, dev, gen):
    """A [D, n] view with leading dimension ld (columns past n hold garbage the kernels must not read)."""
    return torch.randn(D, ld, device=dev, generator=gen)[:, :n]


# ------------------------------------------------------------------------------------------------ kernels vs NumPy
# m covers every instantiation of the update kernel (16 columns per wave: m <= 64, 128, 256, 512, 1024); the last cases
# give blocks of the wide variants several chunks each (grid-stride loop, prefetch of the next chunk)
KERNEL_CASES = [(D, m, b) for D in (1, 5, 1000, 2**20 + 3) for m in (1, 4, 63, 64, 65, 256, 257, 1024)
                for b in (1, 3, 8, 64) if D * (m + b) <= 2**28] + [(2**18 + 3, 256, 8), (2**18 + 3, 300, 3),
                                                                    (2**18 + 3, 1024, 8), (2**18 + 3, 1023, 64)]


@pytest.mark.parametrize("D,m,b", KERNEL_CASES)
def test_basis_kernels(dev, D, m, b):
    gen = torch.Generator(device=dev).manual_seed(D + 7 * m + 131 * b)
    strided = (m + b) % 2 == 1
    Q = _strided(D, m, m + 3, dev, gen) if strided else torch.randn(D, m, device=dev, generator=gen)
    W = _strided(D, b, b + 5, dev, gen) if strided else torch.randn(D, b, device=dev, generator=gen)
    Qn, Wn = Q.double().cpu().numpy(), W.double().cpu().numpy()
    ws = _hip.basis_ws(D, m, b, dev)
    # project: exact products, float64 accumulation -- float32 sums would miss this bound by orders of magnitude
    Cp = _hip.basis_project(Q, W, ws)
    ref = Qn.T @ Wn
    absprod = np.abs(Qn).T @ np.abs(Wn)
    assert np.all(np.abs(Cp.cpu().numpy() - ref) <= 1e-12 * absprod + 1e-300)
    assert torch.equal(Cp, _hip.basis_project(Q, W, ws))   # bit-identical repeat
    # fused update + reproject against update followed by a separate project
    Cc = torch.randn(m, b, device=dev, dtype=torch.float64, generator=gen) / max(m, 1)
    W1, W2 = W.clone(), W.clone()
    C2 = _hip.basis_update(W1, Q, Cc, ws, reproject=True)
    _hip.basis_update(W2, Q, Cc)
    assert torch.equal(W1, W2)
    Wref = Wn - Qn @ Cc.float().double().cpu().numpy()
    scale = 1 + np.abs(Qn).max() * np.abs(Cc.cpu().numpy()).sum(0).max()
    assert np.abs(W1.double().cpu().numpy() - Wref).max() <= 1e-5 * scale
    W1n = W1.double().cpu().numpy()
    assert np.all(np.abs(C2.cpu().numpy() - Qn.T @ W1n) <= 1e-12 * (np.abs(Qn).T @ np.abs(W1n)) + 1e-300)
    # combine, out of place
    Sm = torch.randn(m, b, device=dev, dtype=torch.float64, generator=gen)
    Y = _hip.basis_combine(Q, Sm)
    Yref = Qn @ Sm.float().double().cpu().numpy()
    assert np.abs(Y.double().cpu().numpy() - Yref).max() <= 1e-5 * (1 + np.abs(Qn).max() * np.abs(Sm.cpu().numpy()).sum(0).max())
    torch.cuda.synchronize()


def test_basis_kernels_empty(dev):
    Q = torch.empty(0, 8, device=dev)
    W = torch.empty(0, 4, device=dev)
    ws = _hip.basis_ws(0, 8, 4, dev)
    assert torch.equal(_hip.basis_project(Q, W, ws), torch.zeros(8, 4, device=dev, dtype=torch.float64))
    C2 = _hip.basis_update(W, Q, torch.ones(8, 4, device=dev, dtype=torch.float64), ws, reproject=True)
    assert torch.equal(C2, torch.zeros(8, 4, device=dev, dtype=torch.float64))
    assert _hip.basis_combine(Q, torch.ones(8, 3, device=dev, dtype=torch.float64)).shape == (0, 3)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ operators vs dense f64
def _mlp(dev, dims, rows, act=nn.Tanh, seed=0):
    torch.manual_seed(seed)
    layers = []
    for i in range(len(dims) - 1):
        layers.append(nn.Linear(dims[i], dims[i + 1]))
        if i < len(dims) - 2:
            layers.append(act())
    model = nn.Sequential(*layers).to(dev)
    X, y = torch.rand(rows, dims[0], device=dev), torch.rand(rows, dims[-1], device=dev)
    return model, [(X, y)]


def _dense(op, dev):
    D = op.shape[1]
    cols = [op @ torch.eye(D, device=dev)[:, i: i + 32].contiguous() for i in range(0, D, 32)]
    M = torch.cat(cols, 1).double().cpu().numpy()
    return (M + M.T) / 2


def _check(op, dev, k, which, tol=1e-4):
    lam = np.linalg.eigvalsh(_dense(op, dev))
    w, V = C.eigsh(op, k=k, which=which, tol=tol)
    assert w.device == V.device == op.device and w.dtype == torch.float64 and V.dtype == torch.float32
    top = np.abs(lam).max()
    if which == "LA":
        ref = lam[-k:]
    elif which == "SA":
        ref = lam[:k]
    else:
        ref = np.sort(lam[np.argsort(-np.abs(lam))[:k]])
    wn = w.cpu().numpy()
    # float32 products: eigenvalues to ~tol relative, and never better than the float32 rounding of the operator
    assert np.all(np.abs(wn - ref) <= 2 * tol * np.maximum(np.abs(ref), 2.0**-20 * top) + 1e-5 * top), (wn, ref)
    VtV = (V.T @ V).double().cpu().numpy()
    assert np.abs(VtV - np.eye(k)).max() <= 1e-5
    res = torch.linalg.vector_norm((op @ V) - V * w.float(), dim=0).double().cpu().numpy()
    # the bound as specified; the rounding-noise floor only for eigenvalues that are zero at float32 resolution
    noise = 64 * np.finfo(np.float32).eps * np.abs(wn).max()
    bound = tol * np.maximum(np.abs(wn), 2.0**-20 * np.abs(wn).max())
    assert np.all(res <= np.where(np.abs(wn) <= noise, np.maximum(bound, noise), bound)), (res, wn)


def test_ggn_la_lm(dev):
    model, data = _mlp(dev, [32, 48, 32, 10], 64)
    G = C.GGNLinearOperator(model, nn.MSELoss(), dict(model.named_parameters()), data, check_deterministic=False)
    for which in ("LA", "LM"):
        _check(G, dev, 8, which)


def test_hessian_la_lm_sa(dev):
    model, data = _mlp(dev, [32, 48, 32, 10], 64)
    H = C.HessianLinearOperator(model, nn.MSELoss(), dict(model.named_parameters()), data, check_deterministic=False)
    for which in ("LA", "LM", "SA"):
        _check(H, dev, 6, which)


def test_widest_basis(dev):
    """ncv = 1024: the basis (1016 columns at b = 8) and the residual block fill the kernels' 1024 columns."""
    model, data = _mlp(dev, [32, 48, 32, 10], 64)
    G = C.GGNLinearOperator(model, nn.MSELoss(), dict(model.named_parameters()), data, check_deterministic=False)
    lam = np.linalg.eigvalsh(_dense(G, dev))
    w = C.eigsh(G, k=4, which="LA", ncv=1024, return_eigenvectors=False).cpu().numpy()
    assert np.all(np.abs(w - lam[-4:]) <= 2e-4 * lam[-4:])


def test_zero_start_vector(dev):
    """b = 1 with v0 = 0: the start block has rank 0 and is replaced by a random direction."""
    model, data = _mlp(dev, [32, 48, 32, 10], 64)
    G = C.GGNLinearOperator(model, nn.MSELoss(), dict(model.named_parameters()), data, check_deterministic=False)
    lam = np.linalg.eigvalsh(_dense(G, dev))
    w = C.eigsh(G, k=3, which="LA", block_size=1, v0=torch.zeros(G.shape[0], device=dev),
                return_eigenvectors=False).cpu().numpy()
    assert np.all(np.abs(w - lam[-3:]) <= 2e-4 * lam[-3:])


def test_kfac_lenet5_exact_spectrum(dev):
    """C3: undamped KFAC of LeNet-5 (D = 61 706).  Its spectrum is the union over layers of the products of the two
    factors' eigenvalues, which gives an exact top-k reference without a dense eigh of the operator."""
    from benchmarks.models import lenet5

    torch.manual_seed(0)
    net = lenet5().to(dev)
    X, y = torch.rand(256, 1, 32, 32, device=dev), torch.randint(0, 10, (256,), device=dev)
    K = C.KFACLinearOperator(net, nn.CrossEntropyLoss(), dict(net.named_parameters()), [(X, y)],
                             separate_weight_and_bias=False, check_deterministic=False)
    _, blocks, _ = K
    spectrum = []
    for block in blocks:
        lam = np.ones(1)
        for factor in block:
            lam = np.kron(lam, np.linalg.eigvalsh(factor.double().cpu().numpy()))
        spectrum.append(lam)
    spectrum = np.sort(np.concatenate(spectrum))
    assert spectrum.size == K.shape[0]
    tol = 1e-4
    for which in ("LA", "LM"):
        w, V = C.eigsh(K, k=10, which=which, tol=tol)
        wn = w.cpu().numpy()
        ref = spectrum[-10:] if which == "LA" else np.sort(spectrum[np.argsort(-np.abs(spectrum))[:10]])
        assert np.all(np.abs(wn - ref) <= 2 * tol * np.abs(ref)), (wn, ref)
        res = torch.linalg.vector_norm((K @ V) - V * w.float(), dim=0).double().cpu().numpy()
        assert np.all(res <= tol * np.abs(wn)), (res, wn)
        assert np.abs((V.double().T @ V.double()).cpu().numpy() - np.eye(10)).max() <= 1e-5


def test_rank_deficient_ggn(dev):
    """rows x outputs = 3 x 4 = 12 < k = 16: the nonzero eigenvalues, then zeros at the floor, no NaN."""
    model, data = _mlp(dev, [20, 24, 4], 3)
    G = C.GGNLinearOperator(model, nn.MSELoss(), dict(model.named_parameters()), data, check_deterministic=False)
    lam = np.linalg.eigvalsh(_dense(G, dev))
    w, V = C.eigsh(G, k=16, which="LA")
    assert torch.isfinite(w).all() and torch.isfinite(V).all()
    wn = np.sort(w.cpu().numpy())[::-1]
    top = lam[-1]
    nz = lam[lam > 1e-4 * top][::-1]
    assert len(nz) <= 12
    np.testing.assert_allclose(wn[: len(nz)], nz, rtol=2e-4)
    assert np.abs(wn[len(nz):]).max() <= 1e-5 * top
    assert np.abs((V.T @ V).double().cpu().numpy() - np.eye(16)).max() <= 1e-5


# ------------------------------------------------------------------------------------------------- full size C2
def test_c2_ggn_top10(dev):
    """BASELINE.json configs[1]: MLP 1024-2688-2688-10 (D = 10 010 122), GGN, MSE, one batch of 8."""
    torch.manual_seed(0)
    model = nn.Sequential(nn.Linear(1024, 2688), nn.ReLU(), nn.Linear(2688, 2688), nn.ReLU(), nn.Linear(2688, 10)).to(dev)
    X, y = torch.rand(8, 1024, device=dev), torch.rand(8, 10, device=dev)
    G = C.GGNLinearOperator(model, nn.MSELoss(), dict(model.named_parameters()), [(X, y)], check_deterministic=False)
    tol = 1e-4
    w, V = C.eigsh(G, k=10, which="LA", tol=tol)
    wn = w.cpu().numpy()
    res = torch.linalg.vector_norm((G @ V) - V * w.float(), dim=0).double().cpu().numpy()
    assert np.all(res <= tol * np.abs(wn)), (res, wn)
    assert np.abs((V.double().T @ V.double()).cpu().numpy() - np.eye(10)).max() <= 1e-5   # (float64 sums over 10M rows)
    _, hi = S.approximate_boundaries(G)
    assert abs(wn[-1] - hi) <= 1e-2 * hi
    w2 = C.eigsh(G, k=10, which="LA", tol=tol, return_eigenvectors=False)
    assert torch.equal(w, w2)
