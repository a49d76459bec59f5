"""Host tier (no GPU) of the learned edge masks: the restatement's fixed-order sum against the header's words on cases
small enough to write out, the new option bits in the binding against the header text, every refusal of both bits that
returns before anything is touched (fake device addresses, as ``test_edge_grad_host.py``), the wrappers' own checks, the
parser errors of ``predict`` and the refusals of ``learn_edge_mask`` / ``explanation_fidelity`` on the CPU."""
import argparse
import ctypes

import numpy as np
import pytest
import torch

import c_surface as S
import edge_mask_reference as ref
from primekg_rgcn_linkprediction_amd import DrugDiseaseModel, _lib, attribution, consumers, evaluate, ops, predict

WG, MG, LG = 8, 16, 32
MASK = 1 << 60


# ------------------------------------------------------------------------------------------------ the restatement
def test_the_fixed_order_is_the_headers():
    f = np.float32
    v = np.arange(1, 12, dtype=f) * f(0.1)                     # 11 values: P_0 = v0 + v8, P_1 = v1 + v9, P_2 = v2 + v10
    p = [f(v[0] + v[8]), f(v[1] + v[9]), f(v[2] + v[10]), v[3], v[4], v[5], v[6], v[7]]
    want = f(f(f(p[0] + p[4]) + f(p[2] + p[6])) + f(f(p[1] + p[5]) + f(p[3] + p[7])))
    assert ref.fixed_sum(v) == want
    assert ref.fixed_sum(np.zeros(0, dtype=f)) == 0 and ref.fixed_sum(np.array([3.5], dtype=f)) == f(3.5)
    gen = np.random.default_rng(3)
    v = gen.random(600, dtype=f)                               # past 64: 256 strided sums, a butterfly per 64, three adds
    t = [f(0)] * 256
    for i, x in enumerate(v):
        t[i % 256] = f(t[i % 256] + x)
    w = []
    for wave in range(4):
        lane = t[64 * wave:64 * wave + 64]
        for off in (32, 16, 8, 4, 2, 1):
            lane = [f(lane[i] + lane[i ^ off]) for i in range(64)]
        w.append(lane[0])
    assert ref.fixed_sum(v) == f(f(f(w[0] + w[1]) + w[2]) + w[3])
    assert ref.fixed_sum(v[:65]) != ref.fixed_sum(v[:64]) and ref.fixed_sum(np.ones(131073, dtype=f)) == 131073


def test_the_mask_draw_restated_ones_zeros_nan_and_negative():
    rowptr, perm = np.array([0, 3, 3, 5, 9]), np.array([4, 0, 7, 2, 8, 1, 3, 5, 6])
    ones = np.ones(9, dtype=np.float32)
    w, m, k = ref.mask_draw(rowptr, perm, ones)
    assert k.tolist() == [3, 0, 2, 4] and m.tolist() == [3, 0, 2, 4]
    assert np.array_equal(w[perm], np.float32(1) / np.array([3, 3, 3, 2, 2, 4, 4, 4, 4], dtype=np.float32))
    hidden = np.zeros(9, dtype=bool)
    hidden[[4, 2]] = True
    bad = ones.copy()
    bad[4] = np.nan                                            # hidden: never looked at
    w, m, k = ref.mask_draw(rowptr, perm, bad, hidden)
    assert k.tolist() == [2, 0, 1, 4] and w[4] == 0 and w[2] == 0 and w[0] == np.float32(0.5) and w[8] == 1
    bad[1], bad[0] = np.nan, -0.5                              # a NaN: its whole segment at 0; a negative value: as it is
    w, m, k = ref.mask_draw(rowptr, perm, bad, hidden)
    assert np.isnan(m[3]) and not w[[1, 3, 5, 6]].any() and k[3] == 3
    assert m[0] == np.float32(0.5) and w[0] == -1 and w[7] == 2 and k[0] == 1


def test_the_log_weight_reference_is_the_gradient_in_the_logits_of_a_segment_softmax():
    gen = torch.Generator().manual_seed(2)
    n, r, e, d = 30, 2, 300, 12
    src, dst, rel = (torch.randint(0, hi, (e,), generator=gen) for hi in (n, n, r))
    rowptr, col, perm, seg = ref.G.csr(dst, src, rel, n, r)
    logit = torch.randn(e, dtype=torch.float64, generator=gen).requires_grad_(True)       # per bucketed position
    m = logit.exp()
    w = m / torch.zeros(n * r, dtype=torch.float64).index_add(0, seg, m)[seg]
    x, gagg = torch.randn(n, d, generator=gen), torch.randn(n * r, d, generator=gen)
    agg = torch.zeros(n * r, d, dtype=torch.float64).index_add(0, seg, w.unsqueeze(1) * x.double()[col])
    (agg * gagg.double()).sum().backward()
    w32 = w.detach().float()
    want, bound = ref.log_weight_grad(rowptr, col, w32, x, gagg)
    # (the reference reads the fp32 weights the kernel reads: the float64 softmax differs from them by their rounding)
    assert float((want - logit.grad).abs().max()) <= 4 * ref.U * float(want.abs().max()) * 4
    assert bool((bound > 0).all()) and float(bound.max()) < 1e-4 * float(want.abs().max())
    w0 = w32.clone()
    w0[::4] = 0.0
    out, b0 = ref.log_weight_grad(rowptr, col, w0, x, gagg)
    assert not out[::4].any() and not b0[::4].any()


# ------------------------------------------------------------------------------------------------ the option bits
def test_the_headers_and_the_binding_agree_on_the_new_bits():
    main, drop = S.header_text("rgcn_hip.h"), S.header_text("rgcn_edge_dropout.h")
    assert f"#define RGCN_MODE_LOG_WEIGHT_GRAD {_lib.MODE_LOG_WEIGHT_GRAD} " in main and _lib.MODE_LOG_WEIGHT_GRAD == LG
    assert "#define RGCN_EDGE_DROPOUT_MASK       ((int64_t)1 << 60) " in drop and _lib.EDGE_DROPOUT_MASK == MASK == 1 << 60
    assert len({1, _lib.MODE_SPARSE_ROWS, _lib.MODE_ROW_ORDER, WG, MG, LG}) == 6
    assert len({MASK, _lib.EDGE_DROPOUT_HIDE_TWINS, _lib.EDGE_DROPOUT_PAIRED}) == 3
    assert "edge_dropout" not in main and "#define RGCN_ABI_VERSION 38\n" in main
    for words in ("THE MASK DRAW", "M[s] > 0 ? m(e) / M[s] : 0.0f", "const float mask[E]"):
        assert words in drop
    for words in ("RGCN_MODE_LOG_WEIGHT_GRAD", "w[p] == 0 ? +0.0f : w[p] * (dot[p] - S[s])"):
        assert words in main


A, B, C = S.FAKE_BASE + S.FAKE_STEP, S.FAKE_BASE + 2 * S.FAKE_STEP, S.FAKE_BASE + 3 * S.FAKE_STEP   # x, agg, workspace


def _weighted():
    g = S._fake_graph()
    g.dir[0].weighted = True
    return g


def _call(g=None, transposed=0, x=A, mode=WG | LG, d=64, agg=B, ws=C, ws_bytes=4, first=0, last=-1, job=None, amax=None):
    g = _weighted() if g is None else g
    return _lib.load().rgcn_aggregate_ex(ctypes.addressof(g), transposed, x, mode, d, agg, ws, ws_bytes, first, last, job,
                                         amax, None)


REFUSALS = [
    ("the bit alone", dict(mode=LG), _lib.RGCN_ERR_ARG),
    ("the bit with the mean bit alone", dict(mode=LG | MG), _lib.RGCN_ERR_ARG),
    ("together with the mean mode", dict(mode=WG | MG | LG), _lib.RGCN_ERR_ARG),
    ("fp16 table", dict(mode=WG | LG | 1), _lib.RGCN_ERR_UNSUPPORTED),
    ("sparse rows", dict(mode=WG | LG | _lib.MODE_SPARSE_ROWS), _lib.RGCN_ERR_UNSUPPORTED),
    ("d = 0", dict(d=0), _lib.RGCN_ERR_ARG),
    ("d % 4", dict(d=30), _lib.RGCN_ERR_ARG),
    ("d > 256", dict(d=260), _lib.RGCN_ERR_UNSUPPORTED),
    ("amax", dict(amax=S.FAKE_BASE + 5 * S.FAKE_STEP), _lib.RGCN_ERR_UNSUPPORTED),
    ("direction not built", dict(transposed=1), _lib.RGCN_ERR_ARG),
    ("first level", dict(first=1), _lib.RGCN_ERR_ARG),
    ("last level", dict(last=1), _lib.RGCN_ERR_ARG),
    ("x NULL", dict(x=None), _lib.RGCN_ERR_ARG),
    ("agg NULL", dict(agg=None), _lib.RGCN_ERR_ARG),
    ("workspace NULL", dict(ws=None), _lib.RGCN_ERR_WORKSPACE),
    ("workspace short", dict(ws_bytes=3), _lib.RGCN_ERR_WORKSPACE),
    ("x below 16 bytes", dict(x=A + 4), _lib.RGCN_ERR_ALIGN),
    ("agg below 16 bytes", dict(agg=B + 8), _lib.RGCN_ERR_ALIGN),
    ("workspace below 16 bytes", dict(ws=C + 4, ws_bytes=64), _lib.RGCN_ERR_ALIGN),
]


@pytest.mark.parametrize("what,kwargs,code", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_every_refusal_of_the_log_weight_mode_returns_its_code(what, kwargs, code):
    got = _call(**kwargs)
    assert got == code, f"{what}: code {got} ({_lib.strerror(got)})"


def test_refusals_come_in_the_documented_order():
    job = _lib.SlabJob(splits=1, K1=4, Kc=8, N=4, slab=S.FAKE_BASE + 9 * S.FAKE_STEP, grad_weight=S.FAKE_BASE + 10 * S.FAKE_STEP)
    every = dict(d=260, amax=A, job=ctypes.pointer(job), first=1, x=A + 4, ws_bytes=0)
    mean = S._fake_graph()                                                         # not weighted
    assert _call(mean, mode=LG | 1, **every) == _lib.RGCN_ERR_ARG                  # the bit alone, before the table's format
    assert _call(mean, mode=WG | MG | LG | 1, **every) == _lib.RGCN_ERR_ARG        # both modes, before the table's format
    assert _call(mean, mode=WG | LG | 1, **every) == _lib.RGCN_ERR_UNSUPPORTED
    assert _call(mean, **dict(every, d=30)) == _lib.RGCN_ERR_ARG                   # d % 4 before d > 256
    assert _call(mean, **dict(every, d=64, amax=None)) == _lib.RGCN_ERR_UNSUPPORTED   # the pending job
    assert _call(mean, **dict(every, d=64, amax=None, job=None)) == _lib.RGCN_ERR_ARG  # the levels before the structure
    assert _call(mean, **dict(every, d=64, amax=None, job=None, first=0)) == _lib.RGCN_ERR_UNSUPPORTED   # a mean structure
    assert _call(**dict(every, d=64, amax=None, job=None, first=0)) == _lib.RGCN_ERR_WORKSPACE
    assert _call(**dict(every, d=64, amax=None, job=None, first=0, ws_bytes=4)) == _lib.RGCN_ERR_ALIGN


def test_the_neighbouring_modes_are_what_they_were():
    weighted, mean = _weighted(), S._fake_graph()
    assert _call(weighted, mode=WG | MG) == _lib.RGCN_ERR_UNSUPPORTED              # the mean mode's refusal is not lifted
    assert _call(mean, mode=WG | MG, x=A + 4) == _lib.RGCN_ERR_ALIGN
    assert _call(weighted, mode=WG, x=A + 4) == _lib.RGCN_ERR_ALIGN
    assert _call(mean, mode=WG | LG) == _lib.RGCN_ERR_UNSUPPORTED
    for empty in ("E", "n_key"):
        g = _weighted()
        if empty == "E":
            g.E = 0
        else:
            g.dir[0].n_key = 0
        assert _call(g, x=None, agg=None, ws=None, ws_bytes=0) == _lib.RGCN_OK


def test_the_mask_draw_refuses_before_it_touches_anything():
    """a handle that is only an address: every call below returns before the view is looked at"""
    lib, ed = _lib.load(), S.FAKE_BASE
    call = lambda p, rng, batch, cursor=None, position=None, stats=None: lib.rgcn_edge_dropout_draw(  # noqa: E731
        ed, p, rng, cursor, batch, position, stats, None)
    assert lib.rgcn_edge_dropout_draw(None, 0.0, A, None, MASK, None, None, None) == _lib.RGCN_ERR_ARG
    assert call(0.0, None, MASK) == _lib.RGCN_ERR_ARG                              # the mask is required
    assert call(0.0, A, MASK | (1 << 63)) == _lib.RGCN_ERR_ARG                     # a negative batch
    assert call(0.25, A, MASK) == _lib.RGCN_ERR_ARG                                # p must be 0 ...
    assert call(float("nan"), A, MASK) == _lib.RGCN_ERR_ARG
    assert call(0.25, A + 4, MASK) == _lib.RGCN_ERR_ARG                            # ... before the alignment
    assert call(0.0, A, MASK | _lib.EDGE_DROPOUT_PAIRED) == _lib.RGCN_ERR_ARG      # no word to share
    assert call(0.0, A + 4, MASK) == _lib.RGCN_ERR_ALIGN                           # the 8-byte rule of rng stays
    assert call(0.0, A, MASK | 5, position=B + 4) == _lib.RGCN_ERR_ALIGN
    assert call(0.0, A, MASK, stats=C + 4) == _lib.RGCN_ERR_ALIGN


# ------------------------------------------------------------------------------------------------ the wrappers
class _Alive:
    alive, num_edges, device = True, 100, torch.device("cpu")


def _bare_dropout():
    ed = ops.EdgeDropout.__new__(ops.EdgeDropout)
    ed._handle, ed.graph, ed.device = S.FAKE_BASE, _Alive(), torch.device("cpu")
    return ed


def test_set_mask_checks_before_any_launch_and_draw_keeps_bit_60_out():
    ed = _bare_dropout()
    try:
        with pytest.raises(TypeError):
            ed.set_mask([1.0] * 100)
        with pytest.raises(RuntimeError):
            ed.set_mask(torch.ones(100))                       # no CPU path
        with pytest.raises(ValueError, match="batch"):
            ed.draw(0.0, torch.zeros(2, dtype=torch.int64), batch=1 << 60)
    finally:
        ed._handle = None


def test_through_normalisation_has_no_cpu_path_and_is_not_recordable(monkeypatch):
    with pytest.raises(TypeError):
        ops.aggregate_weight_grad(None, torch.zeros(4, 4), torch.zeros(4, 4), through_normalisation=True)
    monkeypatch.setattr(ops, "_REC", object())
    with pytest.raises(ops._NotRecordable):
        ops.aggregate_weight_grad(None, torch.zeros(4, 4), torch.zeros(4, 4), through_normalisation=True)


# ------------------------------------------------------------------------------------------------ attribution, consumers
def _model(n=12, r=2, **kw):
    return DrugDiseaseModel(n, r, 8, 8, dropout=0.0, **kw)


def test_learn_edge_mask_refuses_on_the_cpu_what_edge_attribution_refuses():
    n, r = 12, 2
    ei, et = torch.randint(0, n, (2, 30)), torch.randint(0, r, (30,))
    model = _model()
    with pytest.raises(ValueError, match="eval"):
        attribution.learn_edge_mask(model, ei, et, 0, 0, 1)
    model.eval()
    with pytest.raises(RuntimeError, match="device"):
        attribution.learn_edge_mask(model, ei, et, 0, 0, 1)
    with pytest.raises(TypeError):
        attribution.learn_edge_mask(model, ei, et, 0, 0, 1, graph=object())
    half = _model(gather_dtype=torch.float16).eval()
    with pytest.raises(NotImplementedError):
        attribution.learn_edge_mask(half, ei, et, 0, 0, 1)
    with pytest.raises(RuntimeError, match="device"):
        consumers.explanation_fidelity(model, ei, et, [(0, 1)], [0], [{"x": [0]}])
    model.train()
    with pytest.raises(ValueError, match="eval"):
        consumers.explanation_fidelity(model, ei, et, [(0, 1)], [0], [{"x": [0]}])


def test_the_receptive_field_is_two_hops_into_the_pair():
    #        0 -> 1 -> 2 (head)     3 -> 4 (tail)     5 -> 6: elsewhere     2 -> 7: out of the head
    ei = torch.tensor([[0, 1, 3, 5, 2, 6], [1, 2, 4, 6, 7, 5]])
    assert attribution.receptive_field(ei, 2, 4, 8).tolist() == [True, True, True, False, False, False]


def test_masked_edges_lists_the_field_by_mask_value():
    ei, et = torch.tensor([[0, 1, 2, 3, 4], [1, 2, 3, 4, 0]]), torch.tensor([0, 1, 0, 1, 0])
    result = {"mask": torch.tensor([0.9, 1.0, 0.2, 0.9, 0.5]), "field": torch.tensor([True, False, True, True, True])}
    got = consumers.masked_edges(result, ei, et, 3)
    assert [e[0] for e in got] == [0, 3, 4] and got[0][:4] == (0, 0, 0, 1) and got[0][4] == pytest.approx(0.9)
    assert consumers.masked_edges(result, ei, et, 0) == [] and len(consumers.masked_edges(result, ei, et, 9)) == 4
    with pytest.raises(ValueError):
        consumers.masked_edges({"mask": result["mask"][:4], "field": result["field"]}, ei, et, 2)


def test_explain_by_mask_and_fidelity_need_relations():
    n, r = 12, 2
    ei, et = torch.randint(0, n, (2, 30)), torch.randint(0, r, (30,))
    ev = evaluate.ModelEvaluator(_model(), {"edge_index": ei[:, :4], "edge_type": et[:4]},
                                 {"edge_index": ei, "edge_type": et, "num_nodes": n}, torch.device("cpu"))
    with pytest.raises(ValueError, match="relations"):
        ev.explain([(0, 1)], by="mask")
    with pytest.raises(ValueError, match="relations"):
        ev.explain([(0, 1)], fidelity=True)
    with pytest.raises(ValueError, match="fidelity must be"):
        ev.explain([(0, 1)], relations=[0], fidelity="some")
    with pytest.raises(ValueError, match="by must be"):
        ev.explain([(0, 1)], by="masks")


BASE = ["--model_path", "m.pt", "--anchors", "1", "--relation", "0"]


def test_predict_flags():
    args = predict.parse_args(BASE)
    assert (args.mask_steps, args.mask_lr, args.explain_fidelity) == (100, 0.1, False)
    args = predict.parse_args(BASE + ["--explain", "5", "--explain_by", "mask", "--explain_edges", "10", "--explain_fidelity",
                                      "--mask_steps", "40", "--mask_lr", "0.2"])
    assert (args.explain, args.explain_by, args.explain_edges, args.explain_fidelity, args.mask_steps, args.mask_lr) == (
        5, "mask", 10, True, 40, 0.2)
    assert predict.parse_args(BASE + ["--explain", "2", "--explain_edges", "3", "--explain_fidelity"]).explain_by == "cosine"
    for bad in (["--explain_by", "mask"], ["--explain_by", "mask", "--explain_edges", "2"],
                ["--explain", "2", "--explain_by", "mask", "--mask_steps", "-1"],
                ["--explain", "2", "--explain_by", "mask", "--mask_lr", "0"],
                ["--explain", "2", "--explain_fidelity"], ["--explain_edges", "2", "--explain_fidelity"],
                ["--explain_edges", "2"], ["--explain_by", "gradient"]):
        with pytest.raises(SystemExit):
            predict.parse_args(BASE + bad)


def test_predict_passes_the_mask_route_and_the_fidelity_on():
    class Evaluator:
        node_class = None

        def top_candidates(self, side, anchors, relations, k, **kw):
            return torch.tensor([[4, 2]]), torch.tensor([[0.5, 0.25]])

        def explain(self, *args, **kwargs):
            self.seen = (args, kwargs)
            graded = [{"cosine": {"full": 1.0, "without": 0.5, "only": 0.9}}] * 2
            if kwargs.get("by") == "cosine":
                return [[], []], [[0] * 4] * 2, graded
            return [[], []], [[0] * 4] * 2, [[(3, 1, 0, 4, 0.75)], []], graded

    ev = Evaluator()
    out = predict.predict(ev, predict.parse_args(BASE + ["--explain", "2", "--explain_by", "mask", "--explain_edges", "1",
                                                         "--mask_steps", "7"]))
    assert ev.seen[1] == {"by": "mask", "relations": [0], "top_edges": 1, "mask_steps": 7, "mask_lr": 0.1}
    assert out["queries"][0]["edges"] == [[[3, 1, 0, 4, 0.75]], []] and "fidelity" not in out["queries"][0]
    assert out["protocol"]["mask"] == {"steps": 7, "lr": 0.1} and "mask value" in out["protocol"]["edges"]["entry"]
    out = predict.predict(ev, predict.parse_args(BASE + ["--explain", "2", "--explain_by", "mask", "--explain_edges", "1",
                                                         "--explain_fidelity"]))
    assert ev.seen[1]["fidelity"] == "all" and out["queries"][0]["fidelity"][0]["cosine"]["without"] == 0.5
    assert out["protocol"]["fidelity"]["explainers"] == ["cosine", "gradient", "mask"]
    out = predict.predict(ev, predict.parse_args(BASE + ["--explain", "2", "--explain_edges", "1", "--explain_fidelity"]))
    assert ev.seen[1]["by"] == "cosine" and "edges" not in out["queries"][0] and len(out["queries"][0]["fidelity"]) == 2


def test_the_planted_toy_separates_in_the_float64_restatement():
    """the condition the GPU test asserts on the device, checked where no device is involved: after 100 steps at the
    defaults the last planted column stands at least 0.2 above the first distractor"""
    import edge_mask_toy as toy
    ei, et, planted = toy.graph()
    model = toy.plant(DrugDiseaseModel(toy.N, toy.R, toy.D, toy.D, dropout=0.0)).eval()
    p = toy.parameters(model)
    lens = torch.bincount(ei[1] * toy.R + et, minlength=toy.N * toy.R)
    assert int(lens[toy.HEAD * toy.R]) == toy.LONG > 64 and len(planted) == 4 and 200 < ei.size(1) < 400
    mask, field, _ = toy.learn_restated(p, ei, et, toy.HEAD, toy.REL, toy.TAIL, toy.N, toy.R, steps=100, lr=0.1,
                                        size_weight=0.005, entropy_weight=1.0)
    assert bool(field[planted].all()) and torch.equal(field, attribution.receptive_field(ei, toy.HEAD, toy.TAIL, toy.N))
    rest = mask.clone()
    rest[planted] = -1.0
    rest[~field] = -1.0
    assert float(mask[planted].min() - rest.max()) >= 0.2
    score = lambda m: float(toy.score_of(p, ei, et, m, toy.HEAD, toy.REL, toy.TAIL, toy.N, toy.R))   # noqa: E731
    only, without = torch.ones_like(mask), torch.ones_like(mask)
    only[field] = 0.0
    only[planted] = 1.0
    without[planted] = 0.0
    assert score(torch.ones_like(mask)) >= 0 and score(only) >= 0 > score(without)
    import inspect
    defaults = {k: v.default for k, v in inspect.signature(attribution.learn_edge_mask).parameters.items()}
    assert (defaults["steps"], defaults["lr"], defaults["size_weight"], defaults["entropy_weight"]) == (100, 0.1, 0.005, 1.0)
