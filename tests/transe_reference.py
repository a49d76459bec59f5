"""The TransE step's contract (``include/rgcn_transe.h``) restated in numpy float64, with the forward-error bounds the GPU
tier holds the device to.  A plain module, not a conftest.

``step`` is the contract: batch-synchronous - every difference from the tables as the step finds them, a row's
contributions summed and applied once, the rows that moved renormalised, all others untouched.  ``step_in_sample_order``
is the reference's loop (``SimpleTransE.fit``, ``src/compare_methods.py:229-270``): the losses of the whole batch first,
then sample by sample on the rows as the earlier samples left them, then EVERY row renormalised.  ``fit`` trains with
either; ``zipf_graph`` is the skewed multigraph the recorded spread (``tests/golden/transe_spread.json``) was taken on.

Bounds (u = 2^-24, the unit roundoff of fp32; |.| elementwise):
  * a contribution of sample i to an entity row is +-2 lr dp_i with dp_i = (E[h] + R[r]) - E[t]; its MAGNITUDE here is
    m_i = 2 lr (|E[h]| + |R[r]| + |E[t]|) - an upper bound of |2 lr dp_i| that also covers the two roundings of forming
    dp_i under cancellation.  Before the normalisation the new row v = row + sum of contributions is held to
    e = 16 u (|row| + sum of magnitudes): n terms added one after the other err by at most u times the sum of the
    |partial sums|, and with 16 the bound holds as long as those stay below 16 times the mean magnitude.
  * through y = v / |v|: dy = dv / |v| - v (v . dv) / |v|^3 to first order, so
    |dy_j| <= e_j / |v| + |v_j| (|v| . e) / |v|^3, plus 16 u |y_j| for the sum of squares (a tree over d terms), the
    square root and the division.  The restatement asserts |e|_2 <= 1e-3 |v|_2 - the regime in which the second-order
    term is below 1 % of the first - and widens the bound by that 1 %.
  * relation rows: 16 u (|R[r]| + sum over the active samples of 2 lr (|E[h]| + |E[t]| + |E[h']| + |E[t']| + 2 |R[r]|)).
  * a sample's loss: 16 u (|a_p|_2 + |a_n|_2 + margin) with a = |E[h]| + |R[r]| + |E[t]| - each norm moves by at most
    the norm of its difference's error (2 u a) and is itself rounded a few times; the mean: the mean of those plus
    16 u times the mean loss for the sum's tree.
  * the active count is exact: the restatement refuses inputs in which some margin + |dp| - |dn| lies within 1e-4 of
    zero without being the exact zero of a corruption that IS its positive (identical operands, identical bits).
"""
from typing import NamedTuple

import numpy as np

U = 2.0 ** -24
NEAR_ZERO = 1e-4


class Step(NamedTuple):
    emb: np.ndarray            # float64 [N, d] after the step
    rel: np.ndarray            # float64 [R, d]
    emb_bound: np.ndarray      # [N, d]: 0 on the rows no active slot names (they keep their bits)
    rel_bound: np.ndarray      # [R, d]
    loss: np.ndarray           # [B]
    loss_mean: float
    loss_mean_bound: float
    active: np.ndarray         # bool [B]
    touched: np.ndarray        # bool [N]: named by a slot of an active sample
    x: np.ndarray              # [B]: margin + |dp| - |dn|


def _split(heads, tails, rels):
    heads, tails, rels = (np.asarray(a, dtype=np.int64) for a in (heads, tails, rels))
    b = heads.size // 2
    assert heads.shape == tails.shape == rels.shape == (2 * b,)
    return b, heads[:b], tails[:b], heads[b:], tails[b:], rels[:b]


def _losses(e, r, h, t, hn, tn, ri, margin):
    dp, dn = e[h] + r[ri] - e[t], e[hn] + r[ri] - e[tn]
    x = margin + np.sqrt((dp * dp).sum(1)) - np.sqrt((dn * dn).sum(1))
    with np.errstate(invalid="ignore"):
        loss = np.where(x <= 0, 0.0, x)                                  # NaN stays NaN
        active = x > 0                                                   # NaN: not active
    return dp, dn, x, loss, active


def step(emb, rel, heads, tails, rels, lr, margin, check_margins=True) -> Step:
    """the contract, batch-synchronous.  ``check_margins``: refuse inputs whose active count hinges on rounding"""
    e, r = np.asarray(emb, dtype=np.float64), np.asarray(rel, dtype=np.float64)
    b, h, t, hn, tn, ri = _split(heads, tails, rels)
    dp, dn, x, loss, active = _losses(e, r, h, t, hn, tn, ri, margin)
    if check_margins:
        same = (h == hn) & (t == tn)
        for i in range(b):
            if np.isnan(x[i]) or (same[i] and x[i] == margin):
                continue
            assert abs(x[i]) > NEAR_ZERO, f"sample {i}: margin + |dp| - |dn| = {x[i]} hinges on rounding"
    ae, ar = np.abs(e), np.abs(r)
    mag_p, mag_n = 2 * lr * (ae[h] + ar[ri] + ae[t]), 2 * lr * (ae[hn] + ar[ri] + ae[tn])
    add, mag = np.zeros_like(e), np.zeros_like(e)
    radd, rmag = np.zeros_like(r), np.zeros_like(r)
    touched = np.zeros(e.shape[0], dtype=bool)
    for i in np.nonzero(active)[0]:
        for row, sign, diff, m in ((h[i], -1, dp[i], mag_p[i]), (t[i], 1, dp[i], mag_p[i]),
                                   (hn[i], 1, dn[i], mag_n[i]), (tn[i], -1, dn[i], mag_n[i])):
            add[row] += sign * 2 * lr * diff
            mag[row] += m
            touched[row] = True
        radd[ri[i]] += 2 * lr * (dp[i] - dn[i])
        rmag[ri[i]] += mag_p[i] + mag_n[i]
    new_e, bound = e.copy(), np.zeros_like(e)
    for row in np.nonzero(touched)[0]:
        v = e[row] + add[row]
        err = 16 * U * (ae[row] + mag[row])
        norm = np.sqrt((v * v).sum())
        with np.errstate(invalid="ignore", divide="ignore"):
            y = v / norm
            if np.isfinite(y).all():
                assert np.sqrt((err * err).sum()) <= 1e-3 * norm, f"row {row}: the update nearly cancels the row"
                bound[row] = 1.01 * (err / norm + np.abs(v) * (np.abs(v) * err).sum() / norm ** 3) + 16 * U * np.abs(y)
        new_e[row] = y
    new_r = r - radd
    rel_bound = 16 * U * (ar + rmag)
    a_p, a_n = mag_p / (2 * lr), mag_n / (2 * lr)
    loss_bound = 16 * U * (np.sqrt((a_p * a_p).sum(1)) + np.sqrt((a_n * a_n).sum(1)) + abs(margin))
    loss_mean = float(loss.mean()) if b else float("nan")
    mean_bound = float(loss_bound.mean() + 16 * U * abs(loss_mean)) if b else 0.0
    return Step(new_e, new_r, bound, rel_bound, loss, loss_mean, mean_bound, active, touched, x)


def step_in_sample_order(emb, rel, heads, tails, rels, lr, margin):
    """the reference's order -> (emb, rel, loss_mean, active count); every row renormalised"""
    e, r = np.array(emb, dtype=np.float64), np.array(rel, dtype=np.float64)
    b, h, t, hn, tn, ri = _split(heads, tails, rels)
    _, _, _, loss, active = _losses(e, r, h, t, hn, tn, ri, margin)
    for i in np.nonzero(active)[0]:
        gp = 2 * lr * (e[h[i]] + r[ri[i]] - e[t[i]])                     # all four gradients before any row is written
        gn = 2 * lr * (e[hn[i]] + r[ri[i]] - e[tn[i]])
        e[h[i]] -= gp
        e[t[i]] += gp
        r[ri[i]] -= gp - gn
        e[hn[i]] += gn
        e[tn[i]] -= gn
    e /= np.sqrt((e * e).sum(1, keepdims=True))
    return e, r, float(loss.mean()), int(active.sum())


def step_synchronous(emb, rel, heads, tails, rels, lr, margin):
    """``step`` in ``step_in_sample_order``'s shape (no bounds, no margin check), vectorised for ``fit``"""
    e, r = np.array(emb, dtype=np.float64), np.array(rel, dtype=np.float64)
    b, h, t, hn, tn, ri = _split(heads, tails, rels)
    dp, dn, _, loss, active = _losses(e, r, h, t, hn, tn, ri, margin)
    w = (2 * lr * active)[:, None]
    add = np.zeros_like(e)
    np.add.at(add, h, -w * dp)
    np.add.at(add, t, w * dp)
    np.add.at(add, hn, w * dn)
    np.add.at(add, tn, -w * dn)
    np.subtract.at(r, ri, w * (dp - dn))
    rows = np.unique(np.concatenate([h[active], t[active], hn[active], tn[active]]))
    v = e[rows] + add[rows]
    e[rows] = v / np.sqrt((v * v).sum(1, keepdims=True))
    return e, r, float(loss.mean()), int(active.sum())


def zipf_graph(num_nodes=1500, num_edges=12000, num_relations=3, seed=0, exponent=0.9):
    """(edge_index int64 [2, E], edge_type int64 [E]): both endpoints drawn with weight ``rank^-exponent``"""
    rng = np.random.RandomState(seed)
    w = np.arange(1, num_nodes + 1, dtype=np.float64) ** -exponent
    w /= w.sum()
    ends = rng.choice(num_nodes, size=(2, num_edges), p=w)
    return ends.astype(np.int64), rng.randint(0, num_relations, size=num_edges).astype(np.int64)


def init_tables(num_nodes, num_relations, d, rng):
    """the reference's start: ``randn * 0.01``, every row of both tables normalised"""
    e, r = rng.randn(num_nodes, d) * 0.01, rng.randn(num_relations, d) * 0.01
    return e / np.sqrt((e * e).sum(1, keepdims=True)), r / np.sqrt((r * r).sum(1, keepdims=True))


def corrupt(h, t, num_nodes, rng):
    """one corruption per positive: a fair coin picks head or tail, a uniform node replaces it"""
    coin, node = rng.rand(h.size) < 0.5, rng.randint(0, num_nodes, size=h.size)
    return np.where(coin, node, h), np.where(coin, t, node)


def fit(edge_index, edge_type, num_nodes, num_relations, d=64, epochs=4, batch=1024, lr=0.01, margin=1.0, seed=0,
        order="sample", max_batches=None):
    """-> (emb, rel, mean of the last epoch's batch losses); ``order``: "sample" (the reference's) or "synchronous" """
    one = {"sample": step_in_sample_order, "synchronous": step_synchronous}[order]
    rng = np.random.RandomState(seed)
    e, r = init_tables(num_nodes, num_relations, d, rng)
    num_edges, done, losses = edge_index.shape[1], 0, []
    batch = min(batch, num_edges)
    for _ in range(epochs):
        losses, perm = [], rng.permutation(num_edges)
        for lo in range(0, num_edges, batch):
            cols = perm[lo:lo + batch]
            h, t, ri = edge_index[0, cols], edge_index[1, cols], edge_type[cols]
            hn, tn = corrupt(h, t, num_nodes, rng)
            e, r, loss, _ = one(e, r, np.concatenate([h, hn]), np.concatenate([t, tn]), np.concatenate([ri, ri]), lr, margin)
            losses.append(loss)
            done += 1
            if max_batches is not None and done >= max_batches:
                return e, r, float(np.mean(losses))
    return e, r, float(np.mean(losses))


def closer_share(emb, rel, edge_index, edge_type, seed=0):
    """the share of the columns whose positive lies closer than one fresh corruption of it"""
    e, r = np.asarray(emb, dtype=np.float64), np.asarray(rel, dtype=np.float64)
    h, t = edge_index
    hn, tn = corrupt(h, t, e.shape[0], np.random.RandomState(seed + 7919))
    dp, dn = e[h] + r[edge_type] - e[t], e[hn] + r[edge_type] - e[tn]
    return float(((dp * dp).sum(1) < (dn * dn).sum(1)).mean())


# ---------------------------------------------------------------------------------------- ranking by TransE distance
def rank_operands(emb, rel, anchor_idx, rel_idx, side):
    """``ops.transe_rank_operands`` in numpy float32: ``(q [B, D], cand [N, D])``"""
    e, r = np.asarray(emb, dtype=np.float32), np.asarray(rel, dtype=np.float32)
    n, d = e.shape
    width = (d + 1 + 31) // 32 * 32
    q, cand = np.zeros((len(anchor_idx), width), np.float32), np.zeros((n, width), np.float32)
    q[:, :d] = e[anchor_idx] + r[rel_idx] if side == "tail" else e[anchor_idx] - r[rel_idx]
    q[:, d] = -0.5
    cand[:, :d] = e
    cand[:, d] = (e * e).sum(1, dtype=np.float32)
    return q, cand


def distances(emb, rel, anchor_idx, rel_idx, side):
    """float64 [B, N]: ``|h + r - e|^2`` over every candidate tail e, or ``|e + r - t|^2`` over every candidate head"""
    e, r = np.asarray(emb, dtype=np.float64), np.asarray(rel, dtype=np.float64)
    q = e[anchor_idx] + r[rel_idx] if side == "tail" else e[anchor_idx] - r[rel_idx]
    diff = q[:, None, :] - e[None, :, :]
    return (diff * diff).sum(2)


def ranks_by_distance(dist, target, eligible=None):
    """``1 + #{eligible n != target : dist[b, n] < dist[b, target]}``: equal distances do not count"""
    b, n = dist.shape
    ok = np.ones((b, n), dtype=bool) if eligible is None else eligible.copy()
    ok[np.arange(b), target] = False
    return 1 + (ok & (dist < dist[np.arange(b), target][:, None])).sum(1)


def topk_by_distance(dist, k, eligible=None):
    """ids int64 [B, k]: distance ascending, equal distances by id ascending, -1 past the eligible candidates"""
    b, n = dist.shape
    ok = np.ones((b, n), dtype=bool) if eligible is None else eligible
    ids = np.full((b, k), -1, dtype=np.int64)
    for i in range(b):
        order = [j for j in np.lexsort((np.arange(n), dist[i])) if ok[i, j]][:k]
        ids[i, :len(order)] = order
    return ids
