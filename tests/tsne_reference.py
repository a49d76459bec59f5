"""Host restatement of ``include/rgcn_tsne.h`` and of ``ops.tsne``'s driver, written from the header's words (numpy, no
device).  Every routine takes a ``dtype``: float64 is what the GPU tier holds the device to (and what the CPU tier holds
to scikit-learn's private helpers); float32 is the same steps in the device's precision - distances and forces formed from
DIFFERENCES, numpy's summation order except for Z, whose order the header fixes - and is used ONLY to measure what that arithmetic costs against float64: the GPU
tier's tolerances are 4 x those errors, on the tests' own inputs.  Also a numpy ``trustworthiness``.
"""
import numpy as np

from cluster_reference import blobs  # noqa: F401  (the fixtures are the cluster tests' Gaussian blobs)

EXPLORATION_ITERS = 250
CHECK_EVERY = 50
TINY32 = float(np.finfo(np.float32).tiny)


# ---------------------------------------------------------------------------------- neighbours
def sqdist_matrix(x, dtype=np.float64):
    """``[M, M]`` squared distances from the differences of the mean-centred rows, summed over the columns in ``dtype``.
    The mean is that of the rows without a NaN or an infinity (of all rows, on finite data): one such row does not
    spread to the others; its own distances are +inf or NaN as the differences give them."""
    x = x.astype(dtype)
    fin = np.isfinite(x).all(1)
    out = np.empty((x.shape[0], x.shape[0]), dtype)
    with np.errstate(invalid="ignore"):
        if fin.any():
            x = x - x[fin].mean(0, dtype=dtype)
        for i in range(x.shape[0]):
            diff = x - x[i]
            out[i] = (diff * diff).sum(1, dtype=dtype)
    return out


def selection_key_sqdist(x, dtype=np.float32):
    """what the selection pass orders by, as a squared distance: ``|xc_i|^2 - 2 (<xc_i, xc_j> - |xc_j|^2 / 2)`` with the
    bracket in ``dtype`` (the augmented-row score) and the row's own constant exact"""
    xc = x.astype(dtype)
    fin = np.isfinite(xc).all(1)
    xc = xc - (xc[fin] if fin.any() else xc).mean(0, dtype=dtype)   # the mean of the finite rows, as sqdist_matrix
    sq = (xc * xc).sum(1, dtype=dtype)
    score = xc @ xc.T + (sq * dtype(-0.5))[None, :]
    return (xc.astype(np.float64) ** 2).sum(1)[:, None] - 2.0 * score.astype(np.float64)


def knn(x, k, dtype=np.float64):
    """``(ids [M, k], sqdist [M, k])``: the k nearest other rows, every row ordered by ``(sqdist, id)``; a NaN distance
    orders as +inf (equal to an infinite one: the id decides) and is returned as it is"""
    d2 = sqdist_matrix(x, dtype)
    key = np.where(np.isnan(d2), np.inf, d2)
    m = d2.shape[0]
    ids = np.empty((m, k), np.int64)
    for i in range(m):
        others = np.delete(np.arange(m), i)
        order = others[np.lexsort((others, key[i, others]))]
        ids[i] = order[:k]
    return ids, np.take_along_axis(d2, ids, 1)


# ---------------------------------------------------------------------------------- affinities
def binary_search(sqdist, perplexity, steps=100, tol=1e-5):
    """scikit-learn's ``_binary_search_perplexity`` on all rows at once, in double.  -> ``(cond_p float64 [M, k], beta
    [M], margin, n_steps [M])``; ``margin`` is the least ``| |H - log perplexity| - tol |`` any row met at any step: how
    far every stop / go-on decision was from flipping."""
    d = np.asarray(sqdist, dtype=np.float64)
    m, _ = d.shape
    target = np.log(perplexity)
    beta = np.ones(m)
    lo, hi = np.full(m, -np.inf), np.full(m, np.inf)
    p = np.zeros_like(d)
    live = np.ones(m, bool)
    n_steps = np.zeros(m, np.int64)
    margin = np.inf
    for _ in range(steps):
        idx = np.nonzero(live)[0]
        if idx.size == 0:
            break
        with np.errstate(over="ignore", under="ignore", invalid="ignore"):
            pr = np.exp(-d[idx] * beta[idx, None])
            s = pr.sum(1)
            s[s == 0.0] = 1e-8
            pr = pr / s[:, None]
            h = np.log(s) + beta[idx] * (d[idx] * pr).sum(1)
        p[idx] = pr
        n_steps[idx] += 1
        diff = h - target
        finite = np.isfinite(diff)
        if finite.any():
            margin = min(margin, float(np.abs(np.abs(diff[finite]) - tol).min()))
        stop = np.abs(diff) <= tol
        up = ~stop & (diff > 0.0)
        down = ~stop & ~up
        b = beta[idx]
        iu, idn = idx[up], idx[down]
        lo[iu] = b[up]
        beta[iu] = np.where(hi[iu] == np.inf, b[up] * 2.0, (b[up] + hi[iu]) / 2.0)
        hi[idn] = b[down]
        beta[idn] = np.where(lo[idn] == -np.inf, b[down] / 2.0, (b[down] + lo[idn]) / 2.0)
        live[idx[stop]] = False
    return p, beta, margin, n_steps


def joint(ids, cond_p):
    """symmetric CSR ``(rowptr, col, val float64)`` of ``(C + C^T) / max(sum, eps)``, ``C[i, ids[i, j]] = cond_p[i, j]``"""
    ids = np.asarray(ids, dtype=np.int64)
    m, k = ids.shape
    rows = np.repeat(np.arange(m, dtype=np.int64), k)
    cols = ids.reshape(-1)
    c = np.asarray(cond_p, dtype=np.float64).reshape(-1)
    keys = np.concatenate([rows * m + cols, cols * m + rows])
    uniq, inverse = np.unique(keys, return_inverse=True)
    val = np.zeros(uniq.size)
    np.add.at(val, inverse, np.concatenate([c, c]))
    val /= max(val.sum(), np.finfo(np.float64).eps)
    rowptr = np.zeros(m + 1, np.int64)
    rowptr[1:] = np.cumsum(np.bincount(uniq // m, minlength=m))
    return rowptr, (uniq % m).astype(np.int64), val


def dense(rowptr, col, val, m):
    out = np.zeros((m, m))
    out[np.repeat(np.arange(m), np.diff(rowptr)), col] = val
    return out


# ---------------------------------------------------------------------------------- one gradient, one update
def _z_rows_in_header_order(q):
    """the row sums of ``q`` (float32, zero diagonal) as the header forms them: per 256 columns eight float32 chains - chain
    u takes columns u, u + 8, ... - added in a fixed tree; the blocks of a row in double"""
    m = q.shape[0]
    total = np.zeros(m, np.float64)
    for t0 in range(0, m, 256):
        tile = q[:, t0:t0 + 256]
        n = tile.shape[1]
        c = np.zeros((m, 8), np.float32)
        for j in range(0, n - n % 8, 8):
            c += tile[:, j:j + 8]
        if n % 8:
            c[:, :n % 8] += tile[:, n - n % 8:]
        total += (((c[:, 0] + c[:, 1]) + (c[:, 2] + c[:, 3])) + ((c[:, 4] + c[:, 5]) + (c[:, 6] + c[:, 7]))).astype(np.float64)
    return total


def gradient(y, rowptr, col, val, exaggeration=1.0, dtype=np.float64, compute_error=True):
    """-> ``(grad [M, 2] in dtype, Z float, kl float or None)``, by the header's formulas"""
    y = y.astype(dtype)
    m = y.shape[0]
    one, ex = dtype(1), dtype(exaggeration)
    dx = y[:, None, 0] - y[None, :, 0]
    dy = y[:, None, 1] - y[None, :, 1]
    q = one / (one + (dx * dx + dy * dy))
    np.fill_diagonal(q, 0)
    z = float(q.astype(np.float64).sum()) if dtype == np.float64 else float(_z_rows_in_header_order(q).sum())
    q2 = q * q
    rep = np.stack([(q2 * dx).sum(1, dtype=dtype), (q2 * dy).sum(1, dtype=dtype)], 1)
    rows = np.repeat(np.arange(m), np.diff(rowptr))
    p = np.asarray(val).astype(dtype)
    qe, dxe, dye = q[rows, col], dx[rows, col], dy[rows, col]
    w = p * qe
    attr = np.zeros((m, 2), dtype)
    full = np.diff(rowptr) > 0                                  # (reduceat hands back an element for an empty segment)
    if len(w):
        starts = np.minimum(rowptr[:-1], len(w) - 1)
        attr[:, 0] = np.where(full, np.add.reduceat(w * dxe, starts), 0)
        attr[:, 1] = np.where(full, np.add.reduceat(w * dye, starts), 0)
    grad = dtype(4) * (ex * attr - (rep.astype(np.float64) / z).astype(dtype))
    kl = None
    if compute_error:
        pe = (ex * p).astype(np.float64)
        kl = float((pe * np.log(np.maximum(pe, TINY32) / np.maximum(qe.astype(np.float64) / z, TINY32))).sum())
    return grad.astype(dtype), z, kl


def update(grad, y, upd, gains, momentum, lr, min_gain=0.01, dtype=np.float64):
    """scikit-learn's ``_gradient_descent`` body -> ``(y, update, gains, |g|^2)``; nothing is changed in place"""
    grad, y, upd, gains = (a.astype(dtype) for a in (grad, y, upd, gains))
    inc = upd * grad < 0
    gains = np.where(inc, gains + dtype(0.2), gains * dtype(0.8))
    gains = np.maximum(gains, dtype(min_gain))
    g = grad * gains
    upd = dtype(momentum) * upd - dtype(lr) * g
    return y + upd, upd, gains, float((g.astype(np.float64) ** 2).sum())


# ---------------------------------------------------------------------------------- the driver
def pca_init(x):
    x = x.astype(np.float64)
    xc = x - x.mean(0)
    _, vec = np.linalg.eigh(xc.T @ xc / max(x.shape[0] - 1, 1))
    comp = vec[:, -2:][:, ::-1].T.copy()
    big = np.abs(comp).argmax(1)
    comp *= np.sign(comp[np.arange(2), big])[:, None]
    y = (xc @ comp.T).astype(np.float32)
    return y / np.std(y[:, 0]) * np.float32(1e-4)


def learning_rate(m, early_exaggeration=12.0):
    return max(m / early_exaggeration / 4.0, 50.0)


def affinities(x, perplexity, dtype=np.float64):
    """rows -> the joint CSR P, through ``knn``, ``binary_search`` (on the distances rounded to float32, as the device
    hands them over) and ``joint``"""
    k = min(x.shape[0] - 1, int(3.0 * perplexity + 1))
    ids, d2 = knn(x, k, dtype)
    cond_p, _, _, _ = binary_search(d2.astype(np.float32), perplexity)
    return joint(ids, cond_p.astype(np.float32))


def run(p, y0, max_iter=1000, early_exaggeration=12.0, lr=None, n_iter_without_progress=300, min_grad_norm=1e-7,
        dtype=np.float64):
    """``ops.tsne``'s two stages from the joint CSR ``p`` and the start ``y0`` -> ``(y, kl, n_iter)``"""
    rowptr, col, val = p
    y = y0.astype(dtype).copy()
    m = y.shape[0]
    lr = learning_rate(m, early_exaggeration) if lr is None else lr
    upd, gains = np.zeros_like(y), np.ones_like(y)
    explore = min(EXPLORATION_ITERS, max_iter)
    error, it = float("nan"), 0
    for last, ex, momentum, patience in ((explore, early_exaggeration, 0.5, EXPLORATION_ITERS),
                                         (max_iter, 1.0, 0.8, n_iter_without_progress)):
        best_error, best_iter = np.inf, it
        for i in range(it, last):
            check = (i + 1) % CHECK_EVERY == 0
            want = check or i == last - 1
            grad, _, kl = gradient(y, rowptr, col, val, ex, dtype, want)
            y, upd, gains, norm2 = update(grad, y, upd, gains, momentum, lr, 0.01, dtype)
            it = i + 1
            if want:
                error = kl
            if check:
                if error < best_error:
                    best_error, best_iter = error, i
                elif i - best_iter > patience:
                    break
                if norm2 ** 0.5 <= min_grad_norm:
                    break
    return y, error, it


# ---------------------------------------------------------------------------------- quality
def trustworthiness(x, y, n_neighbors=5):
    """scikit-learn's ``trustworthiness`` (Euclidean): 1 - the normalised sum, over every point's ``n_neighbors`` nearest
    points in the layout, of how far beyond ``n_neighbors`` their rank in the input space is"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    n = x.shape[0]

    def ordered(a):
        d2 = sqdist_matrix(a)
        np.fill_diagonal(d2, np.inf)
        return np.argsort(d2, axis=1, kind="stable")

    ind_x = ordered(x)
    ind_y = ordered(y)[:, :n_neighbors]
    rank = np.empty((n, n), np.int64)
    rank[np.arange(n)[:, None], ind_x] = np.arange(1, n + 1)[None, :]
    excess = rank[np.arange(n)[:, None], ind_y] - n_neighbors
    t = excess[excess > 0].sum()
    return 1.0 - t * (2.0 / (n * n_neighbors * (2.0 * n - 3.0 * n_neighbors - 1.0)))
