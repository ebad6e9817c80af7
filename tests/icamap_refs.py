"""numpy restatements the embedding-map tests compare with (no GPU, no scikit-learn, no skimage):

* ``fastica_sources``: the pipeline of range_amd/embedding_map.py in plain numpy - standardise, whiten from the
  Gram matrix of the standardised columns (scikit-learn's whiten_solver='eigh' with its sign rule), scikit-learn's
  ``_ica_par`` with the logcosh contrast, unit-variance sources.  ``defect=`` plants one of DEFECTS.
* ``equalize``: skimage.exposure.equalize_hist of a float image (numpy.histogram with nbins bins, bin centres,
  normalised cumulative sum, numpy.interp), with numpy.histogram's uniform-bin rule written out
  (``hist_counts``) so that it can be compared with numpy's own.
* long-double references of the three kernels and their error bounds."""
import numpy as np
from scipy import linalg

DEFECTS = ("drop_row", "double_row", "one_minus_tanh", "keep_mean", "no_sqrt_n", "sign_rule")
TOL = 1e-4
U = 2.0 ** -53


def standardise(X):
    X = np.asarray(X, dtype=np.float64)
    mu = X.mean(0)
    sd = X.std(0)
    sd[sd == 0] = 1e-8
    return (X - mu) / sd, mu, sd


def sym_decorrelation(W):
    s, u = linalg.eigh(np.dot(W, W.T))
    s = np.clip(s, a_min=np.finfo(W.dtype).tiny, a_max=None)
    return np.linalg.multi_dot([u * (1.0 / np.sqrt(s)), u.T, W])


def ica_par(Y, w_init, max_iter=1000, tol=TOL, defect=None):
    """sklearn.decomposition._fastica._ica_par with g = logcosh (alpha = 1) on Y (c, n): (W, n_iter, limits)."""
    W = sym_decorrelation(w_init)
    n = float(Y.shape[1])
    Ys = Y
    if defect == "drop_row":
        Ys = Y[:, :-1]
    elif defect == "double_row":
        Ys = np.concatenate([Y, Y[:, :1]], axis=1)
    limits = []
    for _ in range(max_iter):
        t = np.tanh(np.dot(W, Ys))
        gp = (1 - t if defect == "one_minus_tanh" else 1 - t ** 2).sum(axis=1) / n
        W1 = sym_decorrelation(np.dot(t, Ys.T) / n - gp[:, None] * W)
        lim = max(abs(abs(np.einsum("ij,ij->i", W1, W)) - 1))
        W = W1
        limits.append(float(lim))
        if lim < tol:
            break
    return W, len(limits), np.asarray(limits)


def eig_top(Xs, c):
    """The c largest eigenpairs of Xs^T Xs, descending, and the next eigenvalue (0 when there is none)."""
    lam, u = linalg.eigh(np.dot(Xs.T, Xs))
    lam, u = lam[::-1], u[:, ::-1]
    return lam[:c], u[:, :c], (lam[c] if c < len(lam) else 0.0)


def fastica_sources(X, c=3, seed=2001, max_iter=1000, tol=TOL, defect=None):
    """dict(sources (n, c), n_iter, limits, W, K) of FastICA(n_components=c, random_state=seed,
    whiten='unit-variance', max_iter=max_iter, tol=tol).fit(Xs).transform(Xs), Xs the standardised X."""
    Xs, mu, sd = standardise(X)
    if defect == "keep_mean":
        Xs = Xs + mu / sd
    n = Xs.shape[0]
    lam, u, _ = eig_top(Xs, c)
    sign = np.sign(u[0])
    if defect == "sign_rule":
        sign = np.sign(u[np.abs(u).argmax(axis=0), np.arange(c)])     # (svd_flip's rule instead of FastICA's)
        assert not np.array_equal(sign, np.sign(u[0])), "the fixture does not tell the two sign rules apart"
    u = u * sign
    K = (u / np.sqrt(lam)).T
    Y = np.dot(K, Xs.T)
    if defect != "no_sqrt_n":
        Y = Y * np.sqrt(n)
    w_init = np.random.RandomState(seed).normal(size=(c, c))
    W, n_iter, limits = ica_par(Y, w_init, max_iter, tol, defect)
    S = np.dot(W, np.dot(K, Xs.T)).T
    W = W / np.std(S, axis=0, keepdims=True).T
    return dict(sources=np.dot(Xs, np.dot(W, K).T), n_iter=n_iter, limits=limits, W=W, K=K)


# ---- equalisation ---------------------------------------------------------------------------------------------
def edges_of(x, nbins=256):
    first, last = x.min(), x.max()
    if first == last:
        first, last = first - 0.5, last + 0.5
    return np.linspace(first, last, nbins + 1, dtype=np.float64)


def hist_counts(x, edges):
    """numpy.histogram's rule for uniform bins, written out."""
    nbins = len(edges) - 1
    first, last = edges[0], edges[-1]
    x = x[(x >= first) & (x <= last)]
    idx = (((x - first) / (last - first)) * nbins).astype(np.intp)
    idx[idx == nbins] -= 1
    idx[x < edges[idx]] -= 1
    idx[(x >= edges[idx + 1]) & (idx != nbins - 1)] += 1
    return np.bincount(idx, minlength=nbins).astype(np.int64)


def equalize(x, nbins=256):
    """(out, counts, edges): skimage.exposure.equalize_hist(x, nbins) of a 1-d float64 array."""
    x = np.asarray(x, dtype=np.float64)
    edges = edges_of(x, nbins)
    counts = hist_counts(x, edges)
    centres = (edges[:-1] + edges[1:]) / 2.0
    cdf = counts.cumsum()
    cdf = cdf / float(cdf[-1])
    return np.interp(x, centres, cdf), counts, edges


def equalize_cases():
    """Columns that sit on numpy.histogram's decisions: values on and next to the bin edges, repeated extremes, a
    constant column (range widened by 0.5 either way), two values only, and thirds (inexact quotients)."""
    rng = np.random.default_rng(3)
    x = rng.standard_normal(5000)
    edges = edges_of(x)
    on_edges = np.concatenate([edges, np.nextafter(edges, -np.inf)[1:], np.nextafter(edges, np.inf)[:-1], x[:500]])
    return {"normal": x, "on_edges": on_edges, "extremes": np.array([x.min()] * 7 + [x.max()] * 5 + list(x[:300])),
            "constant": np.full(257, 0.75), "two_values": np.array([1.0, 2.0] * 40), "thirds": np.arange(1000) / 3.0}


# ---- long-double references of the kernels ----------------------------------------------------------------------
def project_ld(X, mean, K):
    """(Y (c, n) long double, bound (c, n)): bound = (d + 2) 2^-53 sum_j |K[k,j] (X[i,j] - mean[j])|."""
    L = np.longdouble
    Z = X.astype(L) - (0 if mean is None else mean.astype(L))
    Y = np.dot(K.astype(L), Z.T)
    mag = np.dot(np.abs(K).astype(L), np.abs(Z).T)
    return Y, (X.shape[1] + 2) * U * mag


def ica_step_ld(Y, W):
    """(A (c, c), b (c,), bound_A, bound_b) in long double: bound = (n + 8) 2^-53 sum_i |term|."""
    L = np.longdouble
    Yl = Y.astype(L)
    u = np.dot(W.astype(L), Yl)
    t = np.tanh(u)
    n = Y.shape[1]
    A = np.dot(t, Yl.T)
    g = 1 / np.cosh(u) ** 2          # = 1 - tanh^2, without the cancellation that would cost the reference its digits
    return A, g.sum(axis=1), (n + 8) * U * np.dot(np.abs(t), np.abs(Yl).T), (n + 8) * U * np.abs(g).sum(axis=1)


def sources_ld(Y, M):
    L = np.longdouble
    S = np.dot(M.astype(L), Y.astype(L)).T
    return S, (Y.shape[0] + 2) * U * np.dot(np.abs(M).astype(L), np.abs(Y).astype(L)).T


def synth_features(n, d, seed):
    """Independent uniform / Laplace / bimodal / exponential sources mixed by a Gaussian matrix, plus 0.05 noise."""
    rng = np.random.default_rng(seed)
    s = np.stack([rng.uniform(-1.7, 1.7, n), rng.laplace(0.0, 0.7, n),
                  rng.choice([-1.0, 1.0], n) + 0.3 * rng.standard_normal(n), rng.exponential(1.0, n) - 1.0], axis=1)
    return np.dot(s, rng.standard_normal((4, d))) + 0.05 * rng.standard_normal((n, d))
