"""Host restatement of ``include/rgcn_cluster.h``, written from the header's words (numpy, no device).

float64: Lloyd's k-means from a given start with the header's rules (equal keys to the lower id, a NaN key never wins,
an empty cluster keeps its centroid and has count 0, a restart stops - and is frozen - when no label changed or
``shift^2 <= tol_abs``, the final labels are the assignment against the final centroids, the inertia comes from the
rows), and the silhouette samples (0 for the only member of a cluster and where ``max(a, b) == 0``, a label nobody
carries is skipped).  These are what the GPU tier holds the device to.

float32 (``dtype=np.float32``): the same steps in the device's arithmetic - keys ``|c|^2 - 2 <x, c>`` and distances
``sqrt(max(0, |x_i|^2 + |x_j|^2 - 2 <x_i, x_j>))`` of rows centred at their mean from fp32 products, fp32 sums (numpy's
summation order, not the matrix core's).  It is used ONLY to measure what that arithmetic costs against float64: the
GPU tier's tolerances are 4 x those errors.
"""
import numpy as np


# ---------------------------------------------------------------------------------- inputs
def blobs(m, d, seed, centres=12, offset=0.0, duplicates=0):
    """Gaussian blobs: ``centres`` centres drawn N(0, 3^2) per coordinate, unit noise, float32 ``[m, d]``; ``offset`` is
    added to every coordinate; the last ``duplicates`` rows repeat the first ones"""
    rng = np.random.default_rng(seed)
    c = rng.normal(0.0, 3.0, size=(centres, d))
    which = rng.integers(0, centres, size=m)
    x = c[which] + rng.normal(0.0, 1.0, size=(m, d)) + offset
    if duplicates:
        x[m - duplicates:] = x[:duplicates]
    return x.astype(np.float32)


def starts(x, k, restarts, seed):
    """``[restarts, k, d]``: k distinct rows of x per restart, seeded"""
    rng = np.random.default_rng(seed)
    return np.stack([x[rng.permutation(x.shape[0])[:k]] for _ in range(restarts)]).astype(np.float32)


# ---------------------------------------------------------------------------------- k-means
def keys(x, c, dtype=np.float64):
    """``[M, k]``: ``|c|^2 - 2 <x, c>`` in ``dtype``; NaN -> +inf (a NaN key never wins)"""
    x, c = x.astype(dtype), c.astype(dtype)
    key = (c * c).sum(1, dtype=dtype)[None, :] - dtype(2) * (x @ c.T)
    return np.where(np.isnan(key), np.inf, key)


def assign(x, c, dtype=np.float64):
    """labels (equal keys to the lower id: ``argmin`` takes the first) and the best-two margin of every row"""
    key = keys(x, c, dtype)
    labels = key.argmin(1)
    two = np.partition(key, 1, axis=1)[:, :2] if key.shape[1] > 1 else np.concatenate([key, key], 1)
    return labels, two[:, 1] - two[:, 0]


def update(x, c, labels, dtype=np.float64):
    """-> (new centroids, counts): the mean of the members; an empty cluster keeps its centroid"""
    k = c.shape[0]
    new = c.astype(dtype).copy()
    counts = np.bincount(labels, minlength=k)
    for j in range(k):
        if counts[j]:
            new[j] = x[labels == j].astype(dtype).sum(0, dtype=dtype) / dtype(counts[j])
    return new, counts


def inertia(x, c, labels, dtype=np.float64):
    diff = x.astype(dtype) - c.astype(dtype)[labels]
    return float((diff * diff).sum(1, dtype=dtype).sum(dtype=dtype))


def tol_abs(x, tol):
    """scikit-learn's: ``tol * mean(var(x, axis 0))``"""
    return float(tol) * float(np.var(x.astype(np.float64), axis=0).mean())


def lloyd(x, init, tol_abs_=0.0, max_iter=300, dtype=np.float64):
    """one restart -> dict(labels, centers, inertia, n_iter, counts, history): ``history[i]`` the counts after
    iteration i's update"""
    c = init.astype(dtype).copy()
    prev = np.full(x.shape[0], -1)
    history, n_iter = [], 0
    for _ in range(max_iter):
        labels, _ = assign(x, c, dtype)
        changed = int((labels != prev).sum())
        new, counts = update(x, c, labels, dtype)
        shift2 = float(((new - c) ** 2).sum())
        c, prev = new, labels
        n_iter += 1
        history.append(counts)
        if changed == 0 or shift2 <= tol_abs_:
            break
    labels, _ = assign(x, c, dtype)
    return {"labels": labels, "centers": c, "inertia": inertia(x, c, labels, dtype), "n_iter": n_iter,
            "counts": np.bincount(labels, minlength=c.shape[0]), "history": history}


def kmeans(x, init, tol_abs_=0.0, max_iter=300, dtype=np.float64):
    """all restarts of ``init`` ``[R, k, d]``; the winner has the least inertia, ties to the lower index"""
    runs = [lloyd(x, init[r], tol_abs_, max_iter, dtype) for r in range(init.shape[0])]
    best = int(np.argmin([run["inertia"] for run in runs]))
    return best, runs


# ---------------------------------------------------------------------------------- silhouette
def pairwise(x, dtype=np.float64):
    """``[M, M]`` Euclidean distances.  float64: from the differences.  float32: the device's way - rows centred at their
    mean, ``sqrt(max(0, |x_i|^2 + |x_j|^2 - 2 <x_i, x_j>))`` from fp32 products, the diagonal exactly 0"""
    if dtype == np.float64:
        x = x.astype(np.float64)
        d2 = np.empty((x.shape[0], x.shape[0]))
        for i in range(x.shape[0]):
            diff = x - x[i]
            d2[i] = (diff * diff).sum(1)
        return np.sqrt(d2)
    x = x.astype(np.float32)
    x = x - x.mean(0, dtype=np.float32)
    sq = (x * x).sum(1, dtype=np.float32)
    d2 = (sq[:, None] + sq[None, :]) - np.float32(2) * (x @ x.T)
    dist = np.sqrt(np.maximum(d2, np.float32(0)))
    np.fill_diagonal(dist, 0)
    return dist


def silhouette_samples(x, labels, k, dtype=np.float64):
    """``[M]`` in ``dtype``: ``(b - a) / max(a, b)``; 0 for the only member of a cluster, where ``max(a, b) == 0`` and
    where no other label has a member; labels without a member are skipped"""
    dist = pairwise(x, dtype)
    labels = np.asarray(labels)
    counts = np.bincount(labels, minlength=k)
    sums = np.stack([dist[:, labels == c].sum(1, dtype=dtype) if counts[c] else np.zeros(len(labels), dtype) for c in range(k)], 1)
    out = np.zeros(len(labels), dtype)
    for i, own in enumerate(labels):
        if counts[own] <= 1:
            continue
        a = sums[i, own] / dtype(counts[own] - 1)
        others = [sums[i, c] / dtype(counts[c]) for c in range(k) if c != own and counts[c]]
        if not others:
            continue
        b = min(others)
        mx = max(a, b)
        if mx > 0:
            out[i] = (b - a) / mx
    return out


def silhouette_mean(samples):
    """the mean the device forms: the samples as they are, summed in double"""
    return float(np.asarray(samples).astype(np.float64).mean())
