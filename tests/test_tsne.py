"""t-SNE on the GPU (``csrc/tsne.hip``, ``include/rgcn_tsne.h``) against the float64 restatement of the header
(``tsne_reference.py``).

Single steps are pinned, whole runs are held statistically, a trajectory never is: the early phase amplifies rounding
(float64 and float32 restatements of the same steps are a quarter of max|Y| apart after 20 iterations).

Ids, patterns, gains and everything "same bits" are compared exactly.  No tolerance of this file is chosen:

* neighbours: margin and gate of a fixture are 4 x the largest error its fp32 HOST restatement (the selection key on
  centred rows, and the distance from differences) shows against float64;
* affinities: both sides search in double on the same float32 distances, so ``cond_p`` may differ by the rounding to
  float32 and the last bits of ``exp`` / the sums: 4 float32 ulps; the joint values 2 ulps;
* one gradient: ``grad`` (relative to the largest entry), ``z`` and ``kl`` (relative) within 4 x the error of the fp32
  restatement on the same inputs (Z is a sum of M^2 positive terms: the header fixes its order and the restatement
  follows it, so the restatement's error is the device's and not one lucky draw of another order's);
* one update: gains exact, ``update`` and ``y`` 2 ulps (the device may contract to an fma), the norm 1e-6;
* a whole run: the recorded spread of four CPU runs (``golden/tsne_blobs300.json``).

Every figure is printed before it is asserted."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import tsne_reference as R
from conftest import ROOT, need_gpu
from primekg_rgcn_linkprediction_amd import DrugDiseaseModel, consumers, ops, synth
from primekg_rgcn_linkprediction_amd import evaluate as E

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "tsne_blobs300.json")


def _t(a, dev, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.to(device=dev, dtype=dtype) if dtype is not None else t.to(dev)


def _ulps(got, want32):
    """largest distance of ``got`` from the float32 array ``want32`` in units of the latter's spacing"""
    want32 = np.asarray(want32, np.float32)
    return float((np.abs(np.asarray(got, np.float64) - want32.astype(np.float64)) / np.spacing(np.abs(want32)).astype(np.float64)).max())


# ---------------------------------------------------------------------------------- neighbours
# name -> (M, d, k, blobs keywords): every M in {3, 63, 64, 65, 129, 700}, d in {32, 96, 128}, k in {1, 2, 63, 64, 91, 127}
KNN_CASES = {
    "m3_k1": (3, 32, 1, {}), "m3_k2": (3, 96, 2, {}), "m63_k2": (63, 128, 2, {}), "m64_k63": (64, 32, 63, {}),
    "m65_k64": (65, 96, 64, {}), "m65_k63": (65, 32, 63, {}), "m129_k91": (129, 128, 91, {}), "m129_k127": (129, 32, 127, {}),
    "m700_k1": (700, 96, 1, {}), "m700_k64": (700, 128, 64, {}), "m700_k91": (700, 128, 91, {}), "m700_k127": (700, 32, 127, {}),
    "copies_k2": (700, 128, 2, {"copies": 8}), "copies_k91": (129, 96, 91, {"copies": 8}), "offset3": (700, 128, 91, {"offset": 3.0}),
}


@functools.lru_cache(maxsize=None)
def _knn_case(name):
    """rows, the float64 distance matrix, and the fixture's gate: 4 x the fp32 restatement's largest error"""
    m, d, k, kw = KNN_CASES[name]
    kw = dict(kw)
    copies = kw.pop("copies", 0)
    x = R.blobs(m, d, seed=3000 + m + d + k, **kw)
    if copies:
        x[m - (copies - 1):] = x[0]                             # `copies` copies of row 0, itself included
    d64 = R.sqdist_matrix(x)
    err_diff = float(np.abs(R.sqdist_matrix(x, np.float32).astype(np.float64) - d64).max())
    err_key = float(np.abs(R.selection_key_sqdist(x, np.float32) - d64).max())
    return x, d64, 4 * max(err_diff, err_key), (err_diff, err_key)


@pytest.mark.parametrize("name", list(KNN_CASES))
def test_knn_rows_are_the_float64_neighbours(name):
    dev = need_gpu()
    m, d, k, kw = KNN_CASES[name]
    x, d64, gate, errs = _knn_case(name)
    ids, sq = ops.knn(_t(x, dev), k)
    assert ids.dtype == torch.int32 and ids.shape == (m, k) and sq.dtype == torch.float32 and sq.shape == (m, k)
    ids, sq = ids.cpu().numpy().astype(np.int64), sq.cpu().numpy()
    rows = np.arange(m)[:, None]
    worst = float(np.abs(sq.astype(np.float64) - d64[rows, ids]).max())
    print(f"{name}: restatement errors (difference form, selection key) {errs[0]:.3e} {errs[1]:.3e} -> gate {gate:.3e}; device {worst:.3e}")
    assert (ids >= 0).all() and (ids < m).all() and not (ids == rows).any()
    assert all(len(set(r)) == k for r in ids.tolist())
    step = np.diff(sq, axis=1)
    assert (step >= 0).all() and (np.diff(ids, axis=1)[step == 0] > 0).all()      # (sqdist, id) ascending
    assert worst <= gate
    others = d64.copy()
    np.fill_diagonal(others, np.inf)
    kth = np.sort(others, axis=1)[:, k - 1:k]                                     # the true k-th distance of every row
    present = np.zeros((m, m), bool)
    present[rows, ids] = True
    assert present[others < kth - gate].all() and not present[others > kth + gate].any()
    if "copies" in kw:
        dup = [0] + list(range(m - (kw["copies"] - 1), m))
        for i in dup:
            mates = [j for j in dup if j != i][:k]
            assert ids[i, :len(mates)].tolist() == mates and (sq[i, :len(mates)] == 0.0).all()
    again = ops.knn(_t(x, dev), k)
    assert np.array_equal(again[0].cpu().numpy(), ids) and np.array_equal(again[1].cpu().numpy(), sq)


def _knn_gate(x):
    """4 x the fp32 restatement's largest error over the pairs of finite rows, and the float64 distances"""
    d64 = R.sqdist_matrix(x)
    fin = np.isfinite(x).all(1)
    pairs = np.ix_(fin, fin)
    with np.errstate(invalid="ignore"):
        err_diff = float(np.abs(R.sqdist_matrix(x, np.float32).astype(np.float64) - d64)[pairs].max())
        err_key = float(np.abs(R.selection_key_sqdist(x, np.float32) - d64)[pairs].max())
    return d64, 4 * max(err_diff, err_key)


@pytest.mark.parametrize("bad", [0, 63, 64, 129])
def test_knn_orders_a_nan_row_as_infinitely_far(bad):
    """M = 130, d = 32, k = 8, row ``bad`` NaN: a NaN distance orders as +inf.  In every other row's list the row could
    stand only behind all finite-distance neighbours - there are 128 of those, so it is not listed and the list is the
    float64 list of the finite rows (the gates of ``test_knn_rows_are_the_float64_neighbours``); the NaN row's own
    list is the first k other ids, ascending, all at a NaN distance.  Both are the restatement's lists."""
    dev = need_gpu()
    m, d, k = 130, 32, 8
    x = R.blobs(m, d, seed=5130)
    x[bad] = np.nan
    d64, gate = _knn_gate(x)
    ids, sq = ops.knn(_t(x, dev), k)
    ids, sq = ids.cpu().numpy().astype(np.int64), sq.cpu().numpy()
    want_ids, want_sq = R.knn(x, k)
    first = [j for j in range(m) if j != bad][:k]
    assert ids[bad].tolist() == first == want_ids[bad].tolist()
    assert np.isnan(sq[bad]).all() and np.isnan(want_sq[bad]).all()
    rest = np.array([i for i in range(m) if i != bad])
    rows = rest[:, None]
    assert not (ids[rest] == bad).any() and not (want_ids[rest] == bad).any()
    assert (ids[rest] >= 0).all() and (ids[rest] < m).all() and not (ids[rest] == rows).any() and np.isfinite(sq[rest]).all()
    step = np.diff(sq[rest], axis=1)
    assert (step >= 0).all() and (np.diff(ids[rest], axis=1)[step == 0] > 0).all()          # (sqdist, id) ascending
    worst = float(np.abs(sq[rest].astype(np.float64) - d64[rows, ids[rest]]).max())
    others = np.where(np.isnan(d64), np.inf, d64)
    np.fill_diagonal(others, np.inf)
    assert worst <= gate
    kth = np.sort(others[rest], axis=1)[:, k - 1:k]                                # the true k-th distance of every row
    present = np.zeros((m, m), bool)
    present[rows, ids[rest]] = True
    assert present[rest][others[rest] < kth - gate].all() and not present[rest][others[rest] > kth + gate].any()
    # where the first k + 1 distances of a row are further apart than the gate can bridge no order can flip: there the
    # list is the restatement's, id by id
    sure = np.diff(np.sort(others[rest], axis=1)[:, :k + 1], axis=1).min(1) > 2 * gate
    print(f"NaN row {bad}: gate {gate:.3e}, device {worst:.3e}, {int((~sure).sum())} of {rest.size} rows below the margin, "
          f"{int((ids[rest] != want_ids[rest]).any(1).sum())} differ")
    assert (~sure).mean() <= 0.05                                # a condition on the inputs, not a tolerance
    assert np.array_equal(ids[rest][sure], want_ids[rest][sure])
    again = ops.knn(_t(x, dev), k)
    assert np.array_equal(again[0].cpu().numpy(), ids) and np.array_equal(again[1].cpu().numpy(), sq, equal_nan=True)


def test_knn_lists_non_finite_rows_last_by_id_when_the_finite_ones_run_out():
    """M = 12, k = 10, rows 2, 7 and 9 not finite (NaN, one NaN element, one +inf element): a finite row has 8
    finite-distance neighbours, then the two lowest of {2, 7, 9}; a non-finite row lists the first 10 other ids."""
    dev = need_gpu()
    m, d, k = 12, 32, 10
    x = R.blobs(m, d, seed=5012)
    x[2] = np.nan
    x[7, 31] = np.nan
    x[9, 0] = np.inf
    d64, gate = _knn_gate(x)
    ids, sq = ops.knn(_t(x, dev), k)
    ids, sq = ids.cpu().numpy().astype(np.int64), sq.cpu().numpy()
    want_ids, want_sq = R.knn(x, k)
    others = np.where(np.isnan(d64), np.inf, d64)
    np.fill_diagonal(others, np.inf)
    fin = np.isfinite(x).all(1)
    gaps = np.diff(np.sort(others[fin], axis=1)[:, :8], axis=1).min()
    print(f"gate {gate:.3e}, least gap between neighbouring finite distances {gaps:.3e}; lists {ids.tolist()}")
    assert gaps > 2 * gate                                       # a condition on the inputs
    assert np.array_equal(ids, want_ids)
    for i in range(m):
        if fin[i]:
            assert ids[i, 8:].tolist() == [2, 7] and fin[ids[i, :8]].all() and np.isfinite(sq[i, :8]).all()
            assert not np.isfinite(sq[i, 8:]).any()
            assert np.abs(sq[i, :8].astype(np.float64) - want_sq[i, :8]).max() <= gate
        else:
            assert ids[i].tolist() == [j for j in range(m) if j != i][:k] and not np.isfinite(sq[i]).any()
    assert np.array_equal(np.isnan(sq), np.isnan(want_sq)) and np.array_equal(np.isinf(sq), np.isinf(want_sq))


# ---------------------------------------------------------------------------------- affinities
@functools.lru_cache(maxsize=None)
def _device_knn(k):
    dev = need_gpu()
    x = R.blobs(700, 128, seed=3100)
    ids, sq = ops.knn(_t(x, dev), k)
    return ids, sq


@pytest.mark.parametrize("k", [2, 64, 65, 91, 127])
def test_affinities_and_joint_are_the_float64_search(k):
    dev = need_gpu()
    perplexity = 1.5 if k == 2 else 30.0
    ids, sq = _device_knn(k)
    sq = sq.clone()
    sq[0] = 1e-30                       # all equal: the entropy is log k at every beta, the search runs its 100 steps
    sq[1] = 0.0                         # all zero: the same, with p = 1 throughout
    sq[2, :min(3, k - 1)] = 0.0         # a row that starts with zeros (duplicates)
    sq[3] = 1e30                        # every p underflows: the s == 0 rule
    host = sq.cpu().numpy()
    want, beta, margin, steps = R.binary_search(host, perplexity)
    print(f"k = {k}: closest stop decision {margin:.2e} from its threshold; steps: all-equal {steps[0]}, zeros {steps[1]}, "
          f"1e30 {steps[3]}, others <= {steps[4:].max()}")
    assert margin > 1e-9, "fixture: a stop decision of the restatement is within 1e-9 of its threshold"
    assert steps[0] == 100 and steps[1] == 100 and steps[3] == 100 and (steps[4:] < 100).mean() > 0.9   # (two equal distances at k = 2 never converge either)
    cond_p, dev_beta = ops.tsne_affinities(sq, perplexity)
    got = cond_p.cpu().numpy()
    want32 = want.astype(np.float32)
    u = _ulps(got, want32)
    print(f"k = {k}: cond_p within {u:.2f} float32 ulps; beta within {np.abs(dev_beta.cpu().numpy() / beta.astype(np.float32) - 1).max():.2e}")
    assert got.dtype == np.float32 and u <= 4
    assert np.array_equal(got[0], np.full(k, np.float32(1.0 / k))) and np.array_equal(got[1], got[0])
    assert np.array_equal(dev_beta.cpu().numpy(), beta.astype(np.float32))
    # the joint matrix, from the device's own conditionals on both sides
    rowptr, col, val = ops.tsne_joint(ids, cond_p)
    wr, wc, wv = R.joint(ids.cpu().numpy(), got)
    assert rowptr.dtype == torch.int32 and col.dtype == torch.int32 and val.dtype == torch.float32
    assert np.array_equal(rowptr.cpu().numpy(), wr) and np.array_equal(col.cpu().numpy(), wc)
    assert all(np.all(np.diff(wc[wr[i]:wr[i + 1]]) > 0) for i in range(700))
    uj = _ulps(val.cpu().numpy(), wv.astype(np.float32))
    total = float(val.sum(dtype=torch.float64))
    print(f"k = {k}: joint values within {uj:.2f} ulps, sum {total:.9f}, nnz {len(wc)}")
    assert uj <= 2 and abs(total - 1.0) <= 1e-6
    again = ops.tsne_affinities(sq, perplexity)
    assert torch.equal(again[0], cond_p) and torch.equal(again[1], dev_beta)


# ---------------------------------------------------------------------------------- one gradient
def _csr_of(dense):
    dense = dense / dense.sum()
    m = dense.shape[0]
    mask = dense != 0
    rowptr = np.zeros(m + 1, np.int64)
    rowptr[1:] = np.cumsum(mask.sum(1))
    return rowptr, np.nonzero(mask)[1].astype(np.int64), dense[mask]


@functools.lru_cache(maxsize=None)
def _p(m, kind):
    """the joint P as float32-valued CSR: the restatement's pipeline (perplexity 30) for M >= 255, every pair for M = 2, 3;
    ``hub``: row 0 holds all M - 1 others on top of it"""
    rng = np.random.default_rng(m)
    if m < 255:
        dense = rng.uniform(0.5, 1.0, size=(m, m))
        dense = dense + dense.T
        np.fill_diagonal(dense, 0)
    else:
        x = R.blobs(m, 32, seed=4000 + m)
        dense = R.dense(*R.affinities(x, 30.0), m)
        if kind == "hub":
            w = rng.uniform(0.0, 2.0, size=m) * dense.max()
            w[0] = 0
            dense[0] += w
            dense[:, 0] += w
    rowptr, col, val = _csr_of(dense)
    if kind == "hub":
        assert rowptr[1] - rowptr[0] == m - 1
    return rowptr, col, val.astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def _layout(m, kind):
    rng = np.random.default_rng(5000 + m)
    if kind == "converged":                                    # the end of the exaggerated stage: the tightest clusters
        x = R.blobs(m, 32, seed=4000 + m)
        y, _, _ = R.run(_p(m, "pipe"), R.pca_init(x), 250, dtype=np.float32)
        return y.astype(np.float32)
    if kind == "coincident":
        y = rng.normal(size=(m, 2)).astype(np.float32)
        y[1::7] = y[0:-1:7][:len(y[1::7])]                      # every seventh point sits exactly on its predecessor
        return y
    return (rng.normal(size=(m, 2)) * float(kind)).astype(np.float32)


# (M, layout, P, exaggeration)
GRAD_CASES = [(2, "1", "pipe", 1.0), (3, "1e-4", "pipe", 12.0), (255, "1", "pipe", 1.0), (256, "10", "pipe", 12.0),
              (257, "1e-4", "pipe", 12.0), (257, "1", "hub", 1.0), (700, "1", "pipe", 1.0), (700, "1e-4", "pipe", 12.0),
              (700, "10", "hub", 12.0), (700, "converged", "pipe", 12.0), (700, "converged", "pipe", 1.0),
              (700, "coincident", "pipe", 1.0)]


@pytest.mark.parametrize("m,layout,kind,ex", GRAD_CASES)
def test_one_gradient_is_the_float64_gradient(m, layout, kind, ex):
    dev = need_gpu()
    rowptr, col, val = _p(m, kind)
    y = _layout(m, layout)
    g64, z64, kl64 = R.gradient(y, rowptr, col, val, ex)
    g32, z32, kl32 = R.gradient(y, rowptr, col, val, ex, np.float32)
    top, kl_scale, floor = float(np.abs(g64).max()), abs(kl64), 0.0
    if m == 2:
        # two points: q / Z = p = 1 / 2, so the two terms of the gradient cancel EXACTLY and KL is log 1 = 0: nothing to be
        # relative to.  The scales are then the attractive term's largest entry and sum p' = exaggeration, and what is left of
        # two equal fp32 quantities is held to four roundings of one of them
        top = float(np.abs(4 * ex * 0.5 * (y[0] - y[1]) / (1 + ((y[0] - y[1]) ** 2).sum())).max())
        kl_scale, floor = float(ex), 4 * 2.0 ** -24
        assert g64.max() == 0.0 == g64.min() and kl64 == 0.0
    gates = (max(4 * float(np.abs(g32.astype(np.float64) - g64).max()) / top, floor), 4 * abs(z32 - z64) / z64,
             max(4 * abs(kl32 - kl64) / kl_scale, floor))
    print(f"M {m} {layout} {kind} x{ex:g}: gates (grad / largest entry, z, kl) {gates[0]:.3e} {gates[1]:.3e} {gates[2]:.3e}")
    yd = _t(y, dev)
    csr = (_t(rowptr, dev, torch.int32), _t(col, dev, torch.int32), _t(val, dev, torch.float32))
    first = None
    for slices in (1, 2, 7, 0):
        grad, z, kl = ops.tsne_gradient(yd, *csr, exaggeration=ex, slices=slices)
        assert grad.dtype == torch.float32 and grad.shape == (m, 2) and z.dtype == kl.dtype == torch.float64
        errs = (float(np.abs(grad.cpu().numpy().astype(np.float64) - g64).max()) / top, abs(float(z) - z64) / z64,
                abs(float(kl) - kl64) / kl_scale)
        print(f"    slices {slices}: device {errs[0]:.3e} {errs[1]:.3e} {errs[2]:.3e}")
        assert errs[0] <= gates[0] and errs[1] <= gates[1] and errs[2] <= gates[2]
        again = ops.tsne_gradient(yd, *csr, exaggeration=ex, slices=slices)
        assert all(torch.equal(a, b) for a, b in zip((grad, z, kl), again))        # the same bits on a second call
        sentinel = torch.full((1,), -7.25, dtype=torch.float64, device=dev)
        quiet = ops.tsne_gradient(yd, *csr, exaggeration=ex, slices=slices, compute_error=False, kl=sentinel)
        assert torch.equal(quiet[0], grad) and torch.equal(quiet[1], z) and float(sentinel) == -7.25
        first = first if first is not None else grad
    if layout == "coincident":
        assert np.isfinite(first.cpu().numpy()).all()


# ---------------------------------------------------------------------------------- one update
@pytest.mark.parametrize("m", [2, 257, 700])
def test_one_update_is_numpys_line_by_line(m):
    dev = need_gpu()
    rng = np.random.default_rng(6000 + m)
    grad = rng.normal(size=(m, 2)).astype(np.float32)
    upd = rng.normal(size=(m, 2)).astype(np.float32)
    gains = rng.uniform(0.005, 3.0, size=(m, 2)).astype(np.float32)       # some below min_gain
    y = rng.normal(size=(m, 2)).astype(np.float32) * 10
    grad[0, 0] = upd[0, 0] = 0.0                                           # the only zero product: both factors are zero
    assert ((upd * grad != 0) | ((upd == 0) & (grad == 0))).all() and (upd * grad < 0).any() and (upd * grad > 0).any()
    wy, wu, wg, wn = R.update(grad, y, upd, gains, 0.8, 175.0, 0.01, np.float32)
    yd, ud, gd = _t(y, dev), _t(upd, dev), _t(gains, dev)
    norm2 = ops.tsne_update(_t(grad, dev), yd, ud, gd, 0.8, 175.0, 0.01)
    uu, uy = _ulps(ud.cpu().numpy(), wu), _ulps(yd.cpu().numpy(), wy)
    rel = abs(float(norm2) - wn) / wn
    print(f"M {m}: update within {uu:.2f} ulps, y within {uy:.2f} ulps, |g|^2 relative {rel:.2e}")
    assert np.array_equal(gd.cpu().numpy(), wg) and wg[0, 0] == max(np.float32(gains[0, 0]) * np.float32(0.8), np.float32(0.01))
    assert uu <= 2 and uy <= 2 and rel <= 1e-6


# ---------------------------------------------------------------------------------- a whole run
@functools.lru_cache(maxsize=None)
def _golden():
    golden = json.load(open(GOLDEN))
    kls = [r["kl"] for r in golden["runs"].values()]
    trusts = [r["trustworthiness"] for r in golden["runs"].values()]
    s = golden["setting"]
    x = R.blobs(s["m"], s["d"], seed=s["seed"])
    kl_gate = max(kls) + 3 * (max(kls) - min(kls))
    trust_gate = min(trusts) - 3 * (max(trusts) - min(trusts))
    # the gates cannot be met by accident: a random layout is more than ten spreads beyond both
    assert golden["random_layout"]["kl"] > kl_gate + 10 * (max(kls) - min(kls))
    assert golden["random_layout"]["trustworthiness"] < trust_gate - 10 * (max(trusts) - min(trusts))
    return s, x, kl_gate, trust_gate


def test_a_whole_run_reaches_the_recorded_quality():
    dev = need_gpu()
    s, x, kl_gate, trust_gate = _golden()
    xd = _t(x, dev)
    res = ops.tsne(xd, perplexity=s["perplexity"], init="pca", max_iter=s["max_iter"])
    y = res.y.cpu().numpy()
    trust = R.trustworthiness(x, y, s["trust_neighbors"])
    print(f"pca: KL {res.kl_divergence:.5f} (gate {kl_gate:.5f}), trustworthiness {trust:.5f} (gate {trust_gate:.5f})")
    assert res.n_iter == s["max_iter"] and res.y.shape == (s["m"], 2) and res.y.dtype == torch.float32 and np.isfinite(y).all()
    assert res.kl_divergence <= kl_gate and trust >= trust_gate
    again = ops.tsne(xd, perplexity=s["perplexity"], init="pca", max_iter=s["max_iter"])
    assert torch.equal(again.y, res.y) and again.kl_divergence == res.kl_divergence and again.n_iter == res.n_iter
    layouts = []
    for seed in (1, 2):
        r = ops.tsne(xd, perplexity=s["perplexity"], init="random", seed=seed, max_iter=s["max_iter"])
        t = R.trustworthiness(x, r.y.cpu().numpy(), s["trust_neighbors"])
        print(f"random, seed {seed}: KL {r.kl_divergence:.5f}, trustworthiness {t:.5f}")
        assert r.n_iter == s["max_iter"] and r.kl_divergence <= kl_gate and t >= trust_gate
        layouts.append(r.y)
    assert not torch.equal(layouts[0], layouts[1])
    given = ops.tsne(xd, perplexity=s["perplexity"], init=torch.from_numpy(R.pca_init(x)), max_iter=60)
    assert given.n_iter == 60 and np.isfinite(given.kl_divergence)


# ---------------------------------------------------------------------------------- callers
def _small_evaluator(dev, n=1000):
    torch.manual_seed(0)
    ei, et, n, r = synth.uniform_graph(n, 8000, 3, seed=1)
    model = DrugDiseaseModel(n, r, 64, 128)
    data = {"edge_index": ei, "edge_type": et, "num_nodes": n, "num_relations": r}
    return model, data, E.ModelEvaluator(model, data, data, dev)


def test_reduce_dimensions_through_the_callers():
    dev = need_gpu()
    _, _, ev = _small_evaluator(dev)
    emb = ev.embeddings()
    assert emb.shape == (1000, 128)
    xy, idx = consumers.reduce_dimensions(emb, sample_size=300, random_state=7, max_iter=60)
    np.random.seed(7)
    assert np.array_equal(idx, np.random.choice(1000, size=300, replace=False))
    assert xy.shape == (300, 2) and xy.dtype == torch.float32 and bool(torch.isfinite(xy).all())
    xy2, idx2, res = ev.reduce_dimensions(sample_size=300, random_state=7, return_result=True, max_iter=60)
    assert torch.equal(xy2, xy) and np.array_equal(idx2, idx) and res.n_iter == 60 and np.isfinite(res.kl_divergence)
    everyone, all_idx = ev.reduce_dimensions(max_iter=10)
    assert everyone.shape == (1000, 2) and np.array_equal(all_idx, np.arange(1000)) and bool(torch.isfinite(everyone).all())
    with pytest.raises(NotImplementedError, match="umap"):
        ev.reduce_dimensions(method="umap")


def test_project_cli_writes_both_files(tmp_path):
    import argparse
    dev = need_gpu()
    from primekg_rgcn_linkprediction_amd import project as P
    model, data, _ = _small_evaluator(dev)
    data_dir = tmp_path / "processed"
    data_dir.mkdir()
    for name in ("test_data.pt", "full_graph.pt"):
        torch.save(data, data_dir / name)
    args = argparse.Namespace(embedding_dim=64, hidden_dim=128, dropout=0.5, decoder_dropout=0.1, num_bases=None)
    torch.save({"epoch": 0, "model_state_dict": model.state_dict(), "args": args}, tmp_path / "model.pt")
    cls = (torch.arange(1000) % 3).to(torch.int32)
    np.savez(data_dir / "node_types.npz", node_class=cls.numpy())
    summary = P.main(["--model_path", str(tmp_path / "model.pt"), "--data_dir", str(data_dir), "--node_types",
                      str(data_dir / "node_types.npz"), "--sample_size", "400", "--max_iter", "100", "--seed", "5",
                      "--output_dir", str(tmp_path / "emb")])
    saved = json.loads((tmp_path / "emb" / "projection_summary.json").read_text())
    assert saved == summary and set(saved) == {"protocol", "kl_divergence", "n_iter", "num_points", "seconds"}
    assert saved["n_iter"] == 100 and saved["num_points"] == 400 and np.isfinite(saved["kl_divergence"])
    assert saved["protocol"]["perplexity"] == 30.0 and saved["protocol"]["sample_size"] == 400
    assert set(saved["seconds"]) == {"neighbours", "affinities", "init", "iterations", "total"}
    with np.load(tmp_path / "emb" / "embedding_2d.npz") as z:
        assert z["xy"].shape == (400, 2) and z["xy"].dtype == np.float32 and np.isfinite(z["xy"]).all()
        assert np.array_equal(z["indices"], consumers.sample_indices(1000, 400, 5))
        assert np.array_equal(z["node_class"], cls.numpy()[z["indices"]])
