"""Embedding maps: the FastICA colours of a location encoder's embeddings, on the GPU.

Replaces the reference's range/evaluation/visualize_embeddings.py: embed every location (:99-119),
standardise the columns (:121-125), fit ``FastICA(n_components=3, random_state=2001,
whiten='unit-variance', max_iter=1000)`` and transform (:132-135), histogram-equalise each component
(:138-139, ``skimage.exposure.equalize_hist``) and read the three values as RGB.

Everything that touches the N rows runs in HIP kernels (include/range_map.h and the ridge probe's column
statistics, row scaler and float64 GEMM); the d x d and c x c algebra - the eigen-decomposition of the
standardised Gram matrix, scikit-learn's symmetric decorrelation and convergence limit - is numpy / LAPACK on
the host, one small copy and one synchronisation per iteration.  There is no CPU fallback.

Deviation from the reference: float32 features are widened to float64 first (scikit-learn would run the whole
fit in float32); the result is the float64 fit of the same numbers."""
from __future__ import annotations

import warnings
from typing import Optional

import numpy as np
import torch

MAX_COMPONENTS = 8
SIGMA_FLOOR = 1e-8          # visualize_embeddings.py:123


class ConvergenceWarning(UserWarning):
    """FastICA stopped at max_iter (scikit-learn warns with its own class of this name)."""


def coord_grid(grid_size, split_ids=None, split_of_interest=None):
    """Locations spaced evenly in coordinate space, as visualize_embeddings.py:29-45 produces them: (H*W, 2)
    float32 (lon, lat), row-major over the grid, lon from -180 to 180 along a row, lat from 90 down to -90; with
    ``split_ids`` (H, W) and ``split_of_interest`` only the cells of that split, in the same order."""
    rows, cols = int(grid_size[0]), int(grid_size[1])
    grid = np.empty((rows, cols, 2), dtype=np.float32)
    grid[..., 0] = np.linspace(-180, 180, cols)[None, :]          # float64 values, rounded once on assignment
    grid[..., 1] = np.linspace(90, -90, rows)[:, None]
    if split_ids is None or split_of_interest is None:
        return grid.reshape(rows * cols, 2)
    return grid[np.asarray(split_ids) == split_of_interest]


def check_shape(n: int, d: int, n_components: int) -> None:
    """The refusals that need no data: c outside 1..8, c > D, N < 2."""
    if not isinstance(n_components, (int, np.integer)) or not 1 <= n_components <= MAX_COMPONENTS:
        raise ValueError(f"n_components must be an integer in 1..{MAX_COMPONENTS}, got {n_components!r}")
    if n < 2:
        raise ValueError(f"FastICA needs at least 2 rows, got {n}")          # sklearn: ensure_min_samples=2
    if d < 1 or n_components > d:
        raise ValueError(f"n_components={n_components} exceeds the {d} feature columns")


def check_finite_sums(col_sums: np.ndarray) -> None:
    """A NaN or an infinity anywhere in a column makes that column's sum non-finite: the reference's two
    asserts (visualize_embeddings.py:127-128) from the statistics pass, without a pass of their own."""
    bad = np.flatnonzero(~np.isfinite(col_sums))
    if bad.size:
        raise ValueError(f"the features hold non-finite values (NaN or infinity; first in column {int(bad[0])}, "
                         f"{bad.size} column(s) in all)")


def sym_decorrelation(W: np.ndarray) -> np.ndarray:
    """(W W^T)^(-1/2) W, as sklearn.decomposition._fastica._sym_decorrelation."""
    from scipy import linalg
    s, u = linalg.eigh(np.dot(W, W.T))
    s = np.clip(s, a_min=np.finfo(W.dtype).tiny, a_max=None)
    return np.linalg.multi_dot([u * (1.0 / np.sqrt(s)), u.T, W])


def whitening(G: np.ndarray, n: int, c: int):
    """From the Gram matrix of the centred columns (d x d, lower triangle valid): the column standard
    deviations (0 -> 1e-8) and K' (c x d) with K' (x - mean) = sqrt(n) K xs, where xs is the standardised row
    and K = (u / sqrt(lambda))^T[:c] scikit-learn's whitening matrix of the standardised data (whiten_solver
    'eigh': the c largest eigenpairs of D^-1 G D^-1, each vector multiplied by the sign of its first entry)."""
    from scipy import linalg
    d = G.shape[0]
    G = np.tril(G) + np.tril(G, -1).T
    std = np.sqrt(np.diagonal(G) / n)
    std[std == 0] = SIGMA_FLOOR
    Gs = G / std[:, None] / std[None, :]
    lam, u = linalg.eigh(Gs, subset_by_index=[d - c, d - 1])
    lam, u = lam[::-1], u[:, ::-1]
    eps = np.finfo(np.float64).eps * 10
    if np.any(lam < eps):
        warnings.warn("there are some small singular values: fewer than n_components directions carry variance")
    lam = np.maximum(lam, eps)
    u = u * np.sign(u[0])
    K = (u / np.sqrt(lam)).T
    return std, K, K * (np.sqrt(n) / std)[None, :]


def _device_of(feats, device) -> torch.device:
    if device is None:
        device = feats.device if isinstance(feats, torch.Tensor) and feats.is_cuda else "cuda"
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"range_amd needs a GPU device, got {dev}: there is no CPU fallback")
    if not torch.cuda.is_available():
        raise RuntimeError("no GPU visible: range_amd runs only on MI355X (gfx950); there is no CPU fallback")
    return torch.device("cuda", dev.index if dev.index is not None else torch.cuda.current_device())


def _check_memory(dev: torch.device, n: int, d: int, c: int, resident: int) -> None:
    """Peak device memory is two float64 copies of the features (the matrix and its centred copy) plus the
    c x n projection, the n x c sources and colours; ``resident`` bytes of it are allocated already."""
    need = 2 * n * d * 8 + 4 * n * c * 8 + 2 * d * d * 8 - resident
    free, _ = torch.cuda.mem_get_info(dev)
    if need > free:
        raise ValueError(f"the embedding map of {n} x {d} features needs {need} more bytes of device memory "
                         f"(two float64 copies of the matrix), {free} bytes are free on {dev}")


def ica_colors(feats, n_components: int = 3, seed: int = 2001, max_iter: int = 1000, tol: float = 1e-4,
               nbins: int = 256, device=None, return_info: bool = False):
    """The equalised FastICA sources of ``feats`` (N, D) - a host array or a device tensor, float32 (widened to
    float64 first: a deviation, see the module text) or float64 - as an (N, n_components) float64 host array
    in [0, 1]: for 3 components, the RGB colour of every row.

    ``return_info=True`` also returns a dict: ``n_iter``, ``converged``, ``limits`` (the convergence limit of
    every iteration), ``components_`` (c, D; acts on the standardised features), ``mean_`` and ``std_`` (D,),
    ``sources`` (N, c; before the equalisation).  Non-finite input raises ``ValueError`` - found from the device's
    column sums, the pass the fit needs anyway (a host array is therefore uploaded before it is refused); when the iteration
    does not converge a ``ConvergenceWarning`` is issued and the last W is used, as scikit-learn does."""
    from ._map_native import MAX_BINS, MapEngine
    if not (isinstance(feats, (np.ndarray, torch.Tensor)) and feats.ndim == 2):
        raise ValueError("feats must be a 2-d array or tensor (N, D)")
    n, d = int(feats.shape[0]), int(feats.shape[1])
    c = n_components
    check_shape(n, d, c)
    if not 2 <= nbins <= MAX_BINS:
        raise ValueError(f"nbins must be in 2..{MAX_BINS}, got {nbins}")
    if max_iter < 1:
        raise ValueError("max_iter must be at least 1")
    if isinstance(feats, np.ndarray):
        if feats.dtype not in (np.float32, np.float64):
            raise ValueError(f"feats must be float32 or float64, got {feats.dtype}")
    elif feats.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"feats must be float32 or float64, got {feats.dtype}")
    dev = _device_of(feats, device)
    on_dev = isinstance(feats, torch.Tensor) and feats.device == dev and feats.dtype == torch.float64
    _check_memory(dev, n, d, c, n * d * 8 if on_dev else 0)
    eng = MapEngine(dev)
    try:
        with torch.cuda.device(dev):
            return _fit(eng, dev, feats, n, d, c, seed, max_iter, tol, nbins, return_info)
    finally:
        eng.close()


def _fit(eng, dev, feats, n, d, c, seed, max_iter, tol, nbins, return_info):
    """``ica_colors`` behind its checks, on an open engine with ``dev`` current."""
    X = torch.as_tensor(feats).to(device=dev, dtype=torch.float64)
    if X.stride(1) != 1 or X.stride(0) < d:
        X = X.contiguous()
    # column statistics, centring, Gram matrix (the ridge probe's kernels)
    col_sum = eng.colstats(X)[2].cpu().numpy()
    check_finite_sums(col_sum)
    mean = col_sum / n
    mean_dev = torch.from_numpy(mean).to(dev)
    Zc = eng.scale_rows(X, shift=mean_dev)
    G = eng.gemm(Zc, Zc, trans_a=True, lower_only=True).cpu().numpy()
    del Zc
    std, K, Kp = whitening(G, n, c)
    # the skinny projection: Y = sqrt(n) K xs^T, c x n
    Y = eng.project(X, torch.from_numpy(np.ascontiguousarray(Kp)).to(dev), mean_dev)
    eng.reserve(n, c)
    # parallel FastICA (sklearn _ica_par, logcosh): the sums on the device, the c x c update here
    W = sym_decorrelation(np.random.RandomState(seed).normal(size=(c, c)))
    limits, converged = [], False
    for _ in range(max_iter):
        Ab = eng.ica_step(Y, W).cpu().numpy()
        A, b = Ab[:c * c].reshape(c, c), Ab[c * c:]
        W1 = sym_decorrelation(A / float(n) - (b / float(n))[:, None] * W)
        lim = max(abs(abs(np.einsum("ij,ij->i", W1, W)) - 1))
        W = W1
        limits.append(float(lim))
        if lim < tol:
            converged = True
            break
    if not converged:
        warnings.warn("FastICA did not converge. Consider increasing tolerance or the maximum number of "
                      "iterations.", ConvergenceWarning)
    # sources of unit variance: S = (W K xs^T)^T / std(S), the deviation in two passes
    M = W / np.sqrt(n)
    S0 = eng.sources(Y, M)
    s_mean = eng.colstats(S0)[2] / n
    Sc = eng.scale_rows(S0, shift=s_mean)
    s_std = np.sqrt(np.diagonal(eng.gemm(Sc, Sc, trans_a=True, lower_only=True).cpu().numpy()) / n)
    del Sc, S0
    W = W / s_std[:, None]
    S = eng.sources(Y, W / np.sqrt(n))
    # equalisation, a column at a time
    mn, mx, _ = eng.colstats(S)
    mn, mx = mn.cpu().numpy(), mx.cpu().numpy()
    colors = eng.empty((n, c))
    for k in range(c):
        first, last = (mn[k] - 0.5, mx[k] + 0.5) if mn[k] == mx[k] else (mn[k], mx[k])
        edges = torch.from_numpy(np.linspace(first, last, nbins + 1, dtype=np.float64)).to(dev)
        eng.equalize(S[:, k], edges, out=colors[:, k])
    out = colors.cpu().numpy()
    info = None
    if return_info:
        info = dict(n_iter=len(limits), converged=converged, limits=np.asarray(limits),
                    components_=np.dot(W, K), mean_=mean, std_=std, sources=S.cpu().numpy())
    return (out, info) if return_info else out


def embed_locations(model, locs, batch_size: int = 100000, device=None):
    """(feats, device): ``model``'s embeddings of ``locs`` (N, 2) (lon, lat) as one float64 (N, D) device matrix.  The
    locations are encoded ``batch_size`` at a time (with ``return_device=True`` where the model's forward has it)
    straight into that matrix; ``device`` defaults to the model's engine's.  The loop of ``embedding_map`` and
    ``cluster_map``."""
    import inspect
    locs = np.asarray(locs) if not isinstance(locs, torch.Tensor) else locs
    if locs.ndim != 2 or locs.shape[1] != 2 or locs.shape[0] < 2:
        raise ValueError(f"locs must be (N >= 2, 2) lon/lat pairs, got {tuple(locs.shape)}")
    if batch_size < 1:
        raise ValueError("batch_size must be positive")
    fwd = getattr(model, "forward", model)
    try:
        on_device = "return_device" in inspect.signature(fwd).parameters
    except (TypeError, ValueError):
        on_device = False
    dev = device
    if dev is None:
        eng = getattr(model, "engine", None)
        dev = eng.device if eng is not None else "cuda"
    dev = _device_of(None, dev)
    n = locs.shape[0]
    feats = None
    with torch.no_grad():
        for i in range(0, n, batch_size):
            chunk = locs[i:i + batch_size]
            e = model(chunk, return_device=True) if on_device else model(chunk)
            e = torch.as_tensor(e)
            if feats is None:
                feats = torch.empty((n, e.shape[1]), dtype=torch.float64, device=dev)
            feats[i:i + e.shape[0]].copy_(e)           # (widens float32, uploads a host result)
    return feats, dev


def embedding_map(model, locs, batch_size: int = 100000, **kw):
    """``ica_colors`` of ``model``'s embeddings of ``locs`` (N, 2) (lon, lat), encoded by ``embed_locations`` into the
    one float64 device matrix the fit then runs on.  Keyword arguments go to ``ica_colors``."""
    feats, kw["device"] = embed_locations(model, locs, batch_size, kw.get("device"))
    return ica_colors(feats, **kw)
