"""Host tier (no GPU) of the gather's adjoint in its edge weights (``RGCN_MODE_WEIGHT_GRAD`` / ``RGCN_MODE_MEAN_GRAD`` of
``rgcn_aggregate_ex``, ``include/rgcn_hip.h``): the reference the GPU tests use held to torch autograd, the option bits,
every refusal of the new mode through the fake handle of ``c_surface`` (none of these calls launches anything), and the
host-side pieces of the attribution built on it."""
import argparse
import ctypes

import pytest
import torch

import c_surface as S
import edge_grad_reference as ref
from primekg_rgcn_linkprediction_amd import DrugDiseaseModel, _lib, evaluate, ops, predict

WG, MG = 8, 16


def _multigraph(n=40, r=3, e=400, seed=3):
    gen = torch.Generator().manual_seed(seed)
    src, dst, rel = (torch.randint(0, hi, (e,), generator=gen) for hi in (n, n, r))
    src[:40], dst[:40], rel[:40] = src[40:80], dst[40:80], rel[40:80]        # duplicate columns
    src[80:100] = dst[80:100]                                               # self loops
    dst[dst == 7] = 8                                                       # a node without in-edges
    return src, dst, rel, n, r


def test_the_mean_reference_is_the_gradient_in_the_mask_of_a_mean():
    src, dst, rel, n, r = _multigraph()
    d = 12
    gen = torch.Generator().manual_seed(5)
    x, gagg = torch.randn(n, d, generator=gen), torch.randn(n * r, d, generator=gen)
    rowptr, col, perm, seg = ref.csr(dst, src, rel, n, r)
    assert torch.equal(seg, ref.segments_of(rowptr)) and int((rowptr[1:] - rowptr[:-1]).max()) > 4
    m = torch.ones(src.numel(), dtype=torch.float64, requires_grad=True)       # one mask per bucketed position
    w = m / torch.zeros(n * r, dtype=torch.float64).index_add(0, seg, m)[seg]
    agg = torch.zeros(n * r, d, dtype=torch.float64).index_add(0, seg, w.unsqueeze(1) * x.double()[col])
    (agg * gagg.double()).sum().backward()
    want, bound = ref.mean(rowptr, col, x, gagg)
    assert float((want - m.grad).abs().max()) <= 1e-12 * float(want.abs().max())
    assert bool((bound > 0).all()) and float(bound.max()) < 1e-4 * float(want.abs().max())
    # the plain mode is the gradient in the weights themselves
    wt = torch.full((src.numel(),), 0.5, dtype=torch.float64, requires_grad=True)
    agg = torch.zeros(n * r, d, dtype=torch.float64).index_add(0, seg, wt.unsqueeze(1) * x.double()[col])
    (agg * gagg.double()).sum().backward()
    dots, eps = ref.plain(rowptr, col, x, gagg)
    assert float((dots - wt.grad).abs().max()) <= 1e-12 * float(dots.abs().max())
    # integer tables: the int64 dots are the float64 ones, and the power-of-two rule names the right segments
    xi, gi = torch.randint(-7, 8, (n, d), generator=gen), torch.randint(-7, 8, (n * r, d), generator=gen)
    assert torch.equal(ref.plain_int(rowptr, col, xi, gi).double(), ref.plain(rowptr, col, xi.float(), gi.float())[0])
    out, exact = ref.mean_int_pow2(rowptr, col, xi, gi)
    length = (rowptr[1:] - rowptr[:-1])[seg]
    assert torch.equal(exact, torch.tensor([c in (1, 2, 4, 8, 16, 32) for c in length.tolist()]))
    assert torch.equal(out[length == 1], torch.zeros(int((length == 1).sum())))


def test_the_header_and_the_binding_agree_on_the_option_bits():
    main = S.header_text("rgcn_hip.h")
    assert f"#define RGCN_MODE_WEIGHT_GRAD {_lib.MODE_WEIGHT_GRAD}\n" in main and _lib.MODE_WEIGHT_GRAD == WG
    assert f"#define RGCN_MODE_MEAN_GRAD {_lib.MODE_MEAN_GRAD} " in main and _lib.MODE_MEAN_GRAD == MG
    assert len({1, _lib.MODE_SPARSE_ROWS, _lib.MODE_ROW_ORDER, WG, MG}) == 5


A, B, C = S.FAKE_BASE + S.FAKE_STEP, S.FAKE_BASE + 2 * S.FAKE_STEP, S.FAKE_BASE + 3 * S.FAKE_STEP   # x, agg, workspace


def _call(handle=None, transposed=0, x=A, mode=WG, d=64, agg=B, ws=C, ws_bytes=4, first=0, last=-1, job=None, amax=None):
    return _lib.load().rgcn_aggregate_ex(S.GRAPH if handle is None else handle, transposed, x, mode, d, agg, ws, ws_bytes,
                                         first, last, job, amax, None)


def _pending_job():
    return _lib.SlabJob(splits=1, K1=4, Kc=8, N=4, slab=S.FAKE_BASE + 9 * S.FAKE_STEP, grad_weight=S.FAKE_BASE + 10 * S.FAKE_STEP)


REFUSALS = [
    ("mean without weight grad", dict(mode=MG), _lib.RGCN_ERR_ARG),
    ("fp16 table", dict(mode=WG | 1), _lib.RGCN_ERR_UNSUPPORTED),
    ("fp16 table, mean", dict(mode=WG | MG | 1), _lib.RGCN_ERR_UNSUPPORTED),
    ("sparse rows", dict(mode=WG | _lib.MODE_SPARSE_ROWS), _lib.RGCN_ERR_UNSUPPORTED),
    ("d = 0", dict(d=0), _lib.RGCN_ERR_ARG),
    ("d < 0", dict(d=-4), _lib.RGCN_ERR_ARG),
    ("d % 4", dict(d=30), _lib.RGCN_ERR_ARG),
    ("d > 256", dict(d=260), _lib.RGCN_ERR_UNSUPPORTED),
    ("amax", dict(amax=S.FAKE_BASE + 5 * S.FAKE_STEP), _lib.RGCN_ERR_UNSUPPORTED),
    ("direction not built", dict(transposed=1), _lib.RGCN_ERR_ARG),
    ("first level", dict(first=1), _lib.RGCN_ERR_ARG),
    ("last level", dict(last=1), _lib.RGCN_ERR_ARG),
    ("last level 0", dict(last=0), _lib.RGCN_ERR_ARG),
    ("x NULL", dict(x=None), _lib.RGCN_ERR_ARG),
    ("agg NULL", dict(agg=None), _lib.RGCN_ERR_ARG),
    ("workspace NULL", dict(ws=None), _lib.RGCN_ERR_WORKSPACE),
    ("workspace short", dict(ws_bytes=3), _lib.RGCN_ERR_WORKSPACE),
    ("x below 16 bytes", dict(x=A + 4), _lib.RGCN_ERR_ALIGN),
    ("x below 16 bytes, mean", dict(x=A + 8, mode=WG | MG), _lib.RGCN_ERR_ALIGN),
    ("agg below 16 bytes", dict(agg=B + 8), _lib.RGCN_ERR_ALIGN),
    ("workspace below 16 bytes", dict(ws=C + 4, ws_bytes=64), _lib.RGCN_ERR_ALIGN),
    ("last level = num_levels passes on to the alignment check", dict(last=2, ws=C + 12, ws_bytes=64), _lib.RGCN_ERR_ALIGN),
]


@pytest.mark.parametrize("what,kwargs,code", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_every_refusal_of_the_weight_gradient_mode_returns_its_code(what, kwargs, code):
    got = _call(**kwargs)
    assert got == code, f"{what}: code {got} ({_lib.strerror(got)})"


def test_a_pending_slab_reduction_is_refused_and_an_empty_job_is_not():
    job = _pending_job()
    assert _call(job=ctypes.pointer(job)) == _lib.RGCN_ERR_UNSUPPORTED
    empty = _lib.SlabJob()
    assert _call(job=ctypes.pointer(empty), x=A + 4) == _lib.RGCN_ERR_ALIGN      # nothing pending: on to the last check


def test_refusals_come_in_the_documented_order():
    job = _pending_job()
    every = dict(d=260, amax=A, job=ctypes.pointer(job), first=1, x=A + 4, ws_bytes=0)
    assert _call(mode=MG | 1, **every) == _lib.RGCN_ERR_ARG                       # the mean bit alone
    assert _call(mode=WG | 1, **every) == _lib.RGCN_ERR_UNSUPPORTED               # the table's format
    assert _call(**dict(every, d=30)) == _lib.RGCN_ERR_ARG                        # d % 4 before d > 256 ...
    assert _call(**dict(every, d=64, amax=None, job=None)) == _lib.RGCN_ERR_ARG   # ... the levels before the workspace
    assert _call(**dict(every, d=64, amax=None, job=None, first=0)) == _lib.RGCN_ERR_WORKSPACE
    assert _call(**dict(every, d=64, amax=None, job=None, first=0, ws_bytes=4)) == _lib.RGCN_ERR_ALIGN


def test_the_mean_mode_is_refused_on_a_weighted_structure_and_empty_structures_return_ok():
    g = S._fake_graph()
    g.dir[0].weighted = True
    handle = ctypes.addressof(g)
    assert _call(handle, mode=WG | MG) == _lib.RGCN_ERR_UNSUPPORTED
    assert _call(handle, mode=WG, x=A + 4) == _lib.RGCN_ERR_ALIGN                 # the plain mode takes it
    for empty in ("E", "n_key"):
        g = S._fake_graph()
        if empty == "E":
            g.E = 0
        else:
            g.dir[0].n_key = 0
        for mode in (WG, WG | MG):
            assert _call(ctypes.addressof(g), mode=mode, x=None, agg=None, ws=None, ws_bytes=0) == _lib.RGCN_OK
    assert _lib.load().rgcn_aggregate_ex(None, 0, A, WG, 64, B, C, 4, 0, -1, None, None, None) == _lib.RGCN_ERR_ARG   # no handle


def test_values_below_eight_still_reach_the_gather():
    """the gather's own refusals, through the same entry point, are what they were"""
    assert _call(mode=0, x=A + 4, ws_bytes=1 << 20) == _lib.RGCN_ERR_ALIGN
    assert _call(mode=1, d=12) == _lib.RGCN_ERR_ARG                               # fp16 table: d % 8
    assert _call(mode=0, ws_bytes=0) == _lib.RGCN_ERR_WORKSPACE                   # the fake graph has one partial row


def test_column_entries_names_the_out_entry_of_every_column():
    src, dst, rel, n, _ = _multigraph()
    ei = torch.stack([src, dst])
    pg = ops.PathGraph(ei, rel, n)
    where = {(int(s), int(t)): i for i, (s, t) in enumerate(zip(pg.out_src.tolist(), pg.out_dst.tolist()))}
    assert len(where) == pg.nnz < src.numel()
    got = pg.column_entries(ei)
    assert got.dtype == torch.int64 and got.tolist() == [where[(int(s), int(t))] for s, t in zip(src.tolist(), dst.tolist())]
    assert pg.column_entries(ei[:, :0]).numel() == 0
    absent = next((s, t) for s in range(n) for t in range(n) if (s, t) not in where)
    with pytest.raises(IndexError):
        pg.column_entries(torch.tensor([[absent[0]], [absent[1]]]))
    with pytest.raises(ValueError):
        pg.column_entries(src)


def test_aggregate_weight_grad_has_no_cpu_path_and_is_not_recordable(monkeypatch):
    with pytest.raises(TypeError):
        ops.aggregate_weight_grad(None, torch.zeros(4, 4), torch.zeros(4, 4))
    monkeypatch.setattr(ops, "_REC", object())
    with pytest.raises(ops._NotRecordable):
        ops.aggregate_weight_grad(None, torch.zeros(4, 4), torch.zeros(4, 4))


def test_explain_by_gradient_needs_relations():
    n, r = 12, 2
    model = DrugDiseaseModel(n, r, 8, 8, dropout=0.0)
    ei, et = torch.randint(0, n, (2, 30)), torch.randint(0, r, (30,))
    ev = evaluate.ModelEvaluator(model, {"edge_index": ei[:, :4], "edge_type": et[:4]},
                                 {"edge_index": ei, "edge_type": et, "num_nodes": n}, torch.device("cpu"))
    with pytest.raises(ValueError, match="relations"):
        ev.explain([(0, 1)], by="gradient")
    with pytest.raises(ValueError, match="by must be"):
        ev.explain([(0, 1)], by="saliency")
    with pytest.raises(ValueError, match="one relation per pair"):
        ev.explain([(0, 1), (2, 3), (4, 5)], by="gradient", relations=[0, 1])


BASE = ["--model_path", "m.pt", "--anchors", "1", "--relation", "0"]


def test_predict_flags():
    args = predict.parse_args(BASE)
    assert args.explain_by == "cosine" and args.explain_edges == 0
    args = predict.parse_args(BASE + ["--explain", "3", "--explain_by", "gradient", "--explain_edges", "5"])
    assert (args.explain, args.explain_by, args.explain_edges) == (3, "gradient", 5)
    for bad in (["--explain_edges", "-1"], ["--explain_edges", "2"], ["--explain", "2", "--explain_edges", "2"],
                ["--explain_by", "gradient"], ["--explain_by", "saliency"]):
        with pytest.raises(SystemExit):
            predict.parse_args(BASE + bad)


def test_predict_without_the_new_flags_calls_explain_as_before():
    class Evaluator:
        node_class = None

        def top_candidates(self, side, anchors, relations, k, **kw):
            return torch.tensor([[4, 2]]), torch.tensor([[0.5, 0.25]])

        def explain(self, *args, **kwargs):
            self.seen = (args, kwargs)
            if kwargs.get("by") == "gradient":
                return [[], []], [[0] * 4] * 2, [[(3, 1, 0, 4, -0.5)], []]
            return [[], []], [[0] * 4] * 2

    ev = Evaluator()
    out = predict.predict(ev, argparse.Namespace(anchor_class=None, anchors=[1], relation=0, side="tail", top_k=2, novel=False,
                                                 candidate_class=None, min_score=None, explain=2, max_path_length=3))
    assert ev.seen == (([(1, 4), (1, 2)], 2, 3), {}) and "edges" not in out["queries"][0] and "edges" not in out["protocol"]
    out = predict.predict(ev, predict.parse_args(BASE + ["--explain", "2", "--explain_by", "gradient", "--explain_edges", "1"]))
    assert ev.seen[1] == {"by": "gradient", "relations": [0], "top_edges": 1}
    assert out["queries"][0]["edges"] == [[[3, 1, 0, 4, -0.5]], []] and out["protocol"]["edges"]["per_candidate"] == 1
