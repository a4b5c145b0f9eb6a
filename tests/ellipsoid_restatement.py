"""Plain-numpy restatement of the location error ellipsoids.  It shares no code with the product.

Input: hypo [n_mod][3 n_win], window w in columns 3w, 3w+1, 3w+2; pivots [n_mod][n_piv] or None.  Per window: the mean, the
covariance (divisor n_mod - 1), its eigenvalues in descending order with unit eigenvectors whose component of largest
magnitude is positive, the squared Mahalanobis distance of every sample and its rank-th smallest, q; per window, coordinate
and pivot the correlation coefficient.  Moments are taken in np.longdouble, so the restatement's own rounding is negligible
against the bounds of the device tests; eigh and the results are float64.  A window with a constant coordinate, or whose
smallest eigenvalue is not positive, has NaN eigenvalues, axes, distances and q; a correlation with a constant column is NaN."""
import numpy as np

LD = np.longdouble


def moments(hypo, pivots=None):
    """mean [n_win][3], cov [n_win][3][3], piv_corr [n_win][3][n_piv], const [n_win][3] -- in long double"""
    x = np.asarray(hypo, dtype=np.float64)
    n_mod, n_col = x.shape
    n_win = n_col // 3
    assert n_col == 3 * n_win and n_mod >= 4
    xl = x.astype(LD).reshape(n_mod, n_win, 3)
    mean = xl.sum(axis=0) / LD(n_mod)
    d = xl - mean
    cov = np.einsum("iwa,iwb->wab", d, d) / LD(n_mod - 1)
    const = (x.max(axis=0) == x.min(axis=0)).reshape(n_win, 3)
    n_piv = 0 if pivots is None else np.shape(pivots)[1]
    corr = np.full((n_win, 3, n_piv), np.nan, dtype=LD)
    if n_piv:
        p = np.asarray(pivots, dtype=np.float64)
        pl = p.astype(LD)
        dp = pl - pl.sum(axis=0) / LD(n_mod)
        pconst = p.max(axis=0) == p.min(axis=0)
        for k in range(n_piv):
            if pconst[k]:
                continue
            with np.errstate(invalid="ignore", divide="ignore"):
                c = np.einsum("iwa,i->wa", d, dp[:, k]) / np.sqrt(np.einsum("iwa,iwa->wa", d, d) * (dp[:, k] @ dp[:, k]))
            corr[:, :, k] = np.where(const, LD(np.nan), c)
    return mean, cov, corr, const


def axes_of(cov):
    """lam [3] descending, V [3][3] (column k = unit axis k, largest |component| positive) of one float64 3 x 3 matrix"""
    lam, V = np.linalg.eigh(np.asarray(cov, dtype=np.float64))
    lam, V = lam[::-1].copy(), V[:, ::-1].copy()
    for k in range(3):
        if V[np.argmax(np.abs(V[:, k])), k] < 0:
            V[:, k] = -V[:, k]
    return lam, V


def distances(hypo, w, mean, cov):
    """d2 [n_mod] of window w through an explicit long-double inverse of its covariance (adjugate over determinant)"""
    C = np.asarray(cov, dtype=LD)
    adj = np.empty((3, 3), dtype=LD)
    for i in range(3):
        for j in range(3):
            r = [a for a in range(3) if a != j]
            c = [a for a in range(3) if a != i]
            adj[i, j] = (-1) ** (i + j) * (C[r[0], c[0]] * C[r[1], c[1]] - C[r[0], c[1]] * C[r[1], c[0]])
    det = C[0, 0] * adj[0, 0] + C[0, 1] * adj[1, 0] + C[0, 2] * adj[2, 0]
    inv = adj / det
    d = np.asarray(hypo, dtype=np.float64)[:, 3 * w:3 * w + 3].astype(LD) - np.asarray(mean, dtype=LD)
    return np.einsum("ia,ab,ib->i", d, inv, d)


def ellipsoid(hypo, pivots=None, rank=None, want_d2=False):
    """dict of float64 arrays: mean [n_win][3], cov [n_win][3][3], lam [n_win][3], axes [n_win][3][3], q [n_win] (the
    rank-th smallest d2, 1-based; rank may be a list, q is then [n_win][len(rank)]), piv_corr [n_win][3][n_piv], const
    [n_win][3]; with want_d2 also d2 [n_mod][n_win]"""
    x = np.asarray(hypo, dtype=np.float64)
    n_mod = x.shape[0]
    mean, cov, corr, const = moments(x, pivots)
    n_win = len(mean)
    ranks = [n_mod] if rank is None else list(np.atleast_1d(rank))
    lam = np.full((n_win, 3), np.nan)
    axes = np.full((n_win, 3, 3), np.nan)
    q = np.full((n_win, len(ranks)), np.nan)
    d2 = np.full((n_mod, n_win), np.nan)
    cov64 = cov.astype(np.float64)
    for w in range(n_win):
        if const[w].any():
            continue
        l, V = axes_of(cov64[w])
        if not l[2] > 0:
            continue
        lam[w], axes[w] = l, V
        d2[:, w] = distances(x, w, mean[w], cov[w]).astype(np.float64)
        q[w] = [np.partition(d2[:, w], r - 1)[r - 1] for r in ranks]
    out = {"mean": mean.astype(np.float64), "cov": cov64, "lam": lam, "axes": axes, "q": q[:, 0] if np.ndim(rank) == 0 else q,
           "piv_corr": corr.astype(np.float64), "const": const}
    if want_d2:
        out["d2"] = d2
    return out
