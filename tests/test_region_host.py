"""CPU tier of what a recorded pass (``ops.Region``) and a cached maximum (``ops.set_amax_hint``) stand for, and of who
checks that they still do: a destroyed graph is neither replayed nor served by ``ops.bucket``, ``_Plan.matches`` as a
table, every way a hinted parameter can be rewritten, the out-of-memory fallback, an ``EdgeDropout`` after its parent.
No launch: graphs are made with ``__new__`` over fake handles, plans are stubs, the library is a stub where
``destroy`` would reach it."""
import ctypes
import math
import types
from collections import OrderedDict

import pytest
import torch

from primekg_rgcn_linkprediction_amd import RGCNConv, conv as conv_mod, ops

FAKE = 0x7F0000000000            # fake addresses, never dereferenced


class _Graph(ops.BucketedGraph):
    def __del__(self):           # a fake handle must never reach rgcn_graph_destroy
        pass


def _graph(handle=FAKE):
    g = _Graph.__new__(_Graph)
    g._handle = ctypes.c_void_p(handle) if handle else None
    g.device, g.bipartite, g.weighted_shard = torch.device("cpu"), False, False
    g.num_nodes = g.num_other_nodes = 4
    g.num_relations, g.num_edges = 3, 0
    return g


class _StubLib:
    def __init__(self):
        self.destroyed = []

    def rgcn_graph_destroy(self, handle):
        self.destroyed.append(handle.value)


class _StubPlan(ops._Plan):
    """a plan that says yes to every input and notes that it was issued"""

    def __init__(self, error=None):
        self.calls, self.error = 0, error

    def matches(self, inputs):
        return True

    def run(self, inputs, want, fill=None):
        self.calls += 1
        if self.error is not None:
            raise self.error
        return ["replayed"]


def _levels_pass(x, *, graph):
    graph.num_levels(False)                      # like every wrapper: graph.handle first, then the library
    return (x,)


REGION = ops.Region("test.host", _levels_pass)


def _plant(owner, region=REGION, key="k", plan=None):
    plan = plan if plan is not None else _StubPlan()
    owner.__dict__.setdefault("_regions", {})[(region.name, key, ops.GEMM_PRECISION)] = plan
    return plan


# ---------------------------------------------------------------------------------- hole 1: a destroyed owner
def test_destroy_drops_the_recorded_passes_of_a_graph_and_of_every_graph_it_owns(monkeypatch):
    lib = _StubLib()
    monkeypatch.setattr(ops, "_L", lambda: lib)
    monkeypatch.setattr(ops, "_GRAPH_CACHE", OrderedDict())
    graph, merged, shard, hub = _graph(FAKE), _graph(FAKE + 8), _graph(FAKE + 16), _graph(FAKE + 24)
    graph._merged = merged
    graph.__dict__["_row_blocks"] = {32: [(0, 4, shard)]}
    graph.__dict__["_fused_plans"] = {(16, False): ops.FusedPlan(16, None, None, None, hub, 1, 1),
                                      (16, True): ops.FusedPlan(16, None, None, None, None, 0, 0)}
    graph.__dict__["_mask_ptrs"] = {False: FAKE + 64}
    graph.__dict__["_row_mask_ptrs"] = {False: FAKE + 72}
    plans = [_plant(g) for g in (graph, merged, shard, hub)]
    x = torch.zeros(4, 8)
    assert graph.alive and REGION.run(graph, "k", (x,), dict(graph=graph)) == ["replayed"] and plans[0].calls == 1
    graph.destroy()
    for g in (graph, merged, shard, hub):
        assert "_regions" not in g.__dict__ and not g.alive and g._handle is None
    assert "_mask_ptrs" not in graph.__dict__ and "_row_mask_ptrs" not in graph.__dict__
    assert sorted(lib.destroyed) == [FAKE, FAKE + 8, FAKE + 16, FAKE + 24]
    with pytest.raises(RuntimeError, match="BucketedGraph was destroyed"):
        REGION.run(graph, "k", (x,), dict(graph=graph))
    assert "_regions" not in graph.__dict__, "a call on a destroyed graph started a new record"
    assert [p.calls for p in plans] == [1, 0, 0, 0]
    graph.destroy()                                                     # twice is once
    assert len(lib.destroyed) == 4


def test_a_plan_left_on_a_destroyed_graph_is_not_issued(monkeypatch):
    """belt and braces: whoever puts a plan back (or a destroy that forgot one) still gets the wrappers' error"""
    lib = _StubLib()
    monkeypatch.setattr(ops, "_L", lambda: lib)
    monkeypatch.setattr(ops, "_GRAPH_CACHE", OrderedDict())
    graph = _graph()
    graph.destroy()
    plan = _plant(graph)
    x = torch.zeros(4, 8)
    for _ in range(3):
        with pytest.raises(RuntimeError, match="BucketedGraph was destroyed"):
            REGION.run(graph, "k", (x,), dict(graph=graph))
    assert plan.calls == 0


# ---------------------------------------------------------------------------------- hole 2: bucket() and a destroyed graph
def _cache_key(ei, et, n, r):
    return (ei.data_ptr(), et.data_ptr(), ei._version, et._version, tuple(ei.shape), n, r, str(ei.device))


def test_bucket_never_serves_a_destroyed_graph(monkeypatch):
    cache = OrderedDict()
    monkeypatch.setattr(ops, "_GRAPH_CACHE", cache)
    ei, et = torch.zeros(2, 5, dtype=torch.int64), torch.zeros(5, dtype=torch.int64)
    live = _graph()
    cache[_cache_key(ei, et, 4, 3)] = (live, ei, et)
    assert ops.bucket(ei, et, 4, 3) is live                             # (the key above is the cache's own)
    dead = _graph(None)
    cache[_cache_key(ei, et, 4, 3)] = (dead, ei, et)
    with pytest.raises(RuntimeError, match="edge_index is on cpu.*no CPU fallback"):
        ops.bucket(ei, et, 4, 3)                                        # built again: the constructor refuses CPU columns
    assert not cache, "the entry of a destroyed graph stays in the cache"


def test_destroy_evicts_the_graph_from_the_cache(monkeypatch):
    lib = _StubLib()
    monkeypatch.setattr(ops, "_L", lambda: lib)
    cache = OrderedDict()
    monkeypatch.setattr(ops, "_GRAPH_CACHE", cache)
    ei, et = torch.zeros(2, 5, dtype=torch.int64), torch.zeros(5, dtype=torch.int64)
    a, b = _graph(FAKE), _graph(FAKE + 8)
    cache[_cache_key(ei, et, 4, 3)] = (a, ei, et)
    cache[_cache_key(ei, et, 5, 3)] = (b, ei, et)
    a.destroy()
    assert list(cache) == [_cache_key(ei, et, 5, 3)] and ops.bucket(ei, et, 5, 3) is b
    assert lib.destroyed == [FAKE]


# ---------------------------------------------------------------------------------- _Plan.matches
def _hand_plan(signature, input_bytes, overlaps=()):
    plan = ops._Plan.__new__(ops._Plan)
    plan.signature, plan.input_bytes, plan.overlaps = signature, input_bytes, overlaps
    return plan


A, B = torch.zeros(4, 8), torch.zeros(8)
ARENA = torch.zeros(1024, dtype=torch.uint8)
F32 = torch.float32
MATCH_TABLE = [
    ("the recorded inputs", lambda: [A, None, B], True),
    ("other tensors of the same kind", lambda: [torch.ones(4, 8), None, torch.ones(8)], True),
    ("None where a tensor was recorded", lambda: [None, None, B], False),
    ("a tensor where None was recorded", lambda: [A, B, B], False),
    ("another shape, as many elements", lambda: [torch.zeros(8, 4), None, B], False),
    ("another shape, one row more", lambda: [torch.zeros(5, 8), None, B], False),
    ("float64", lambda: [A.double(), None, B], False),
    ("float16", lambda: [A, None, B.half()], False),
    ("a transposed view of the recorded shape", lambda: [torch.zeros(8, 4).t(), None, B], False),
    ("every second row", lambda: [torch.zeros(8, 8)[::2], None, B], False),
    ("an arena view of the recorded kind", lambda: [ops.Lazy(ARENA, 256, (4, 8), F32), None, B], True),
    ("an arena view of another shape", lambda: [ops.Lazy(ARENA, 256, (8, 4), F32), None, B], False),
    ("an arena view of another type", lambda: [ops.Lazy(ARENA, 256, (4, 8), torch.float16), None, B], False),
    ("an arena view where None was recorded", lambda: [A, ops.Lazy(ARENA, 0, (8,), F32), B], False),
    ("one input fewer", lambda: [A, None], False),
    ("one input more", lambda: [A, None, B, B], False),
    ("no input", lambda: [], False),
    ("the third input inside the first", lambda: [A, None, A[0]], False),
    ("slices of two other allocations, apart", lambda: [torch.zeros(5, 8)[1:], None, A[0]], True),
]


@pytest.mark.parametrize("what,inputs,expect", MATCH_TABLE, ids=[row[0] for row in MATCH_TABLE])
def test_matches_over_a_hand_made_signature(what, inputs, expect):
    plan = _hand_plan([(F32, (4, 8), -1), None, (F32, (8,), -1)], [128, 0, 32])
    assert plan.signature == [ops._signature(t) for t in (A, None, B)]
    assert plan.matches(inputs()) is expect, what


def test_matches_compares_the_device_index():
    here, there = [(F32, (4, 8), -1)], [(F32, (4, 8), 0)]             # (-1: the host; 0: cuda:0)
    assert _hand_plan(here, [128]).matches([A]) and not _hand_plan(there, [128]).matches([A])
    lazy = ops.Lazy(ARENA, 0, (4, 8), F32)
    assert _hand_plan(here, [128]).matches([lazy]) and not _hand_plan(there, [128]).matches([lazy])


def test_matches_compares_how_the_inputs_overlap():
    """a pass recorded while two inputs shared bytes named both after the first: the list is right for calls that
    overlap the same way and for no other"""
    sig, nbytes = [(F32, (4, 8), -1), None, (F32, (8,), -1)], [128, 0, 32]
    assert ops._overlaps([A.data_ptr(), 0, B.data_ptr()], nbytes) == ()
    first_row = ops._overlaps([A.data_ptr(), 0, A[0].data_ptr()], nbytes)
    second_row = ops._overlaps([A.data_ptr(), 0, A[1].data_ptr()], nbytes)
    assert first_row == ((0, 2, 0),) and second_row == ((0, 2, 32),)
    tied = _hand_plan(sig, nbytes, first_row)
    assert tied.matches([A, None, A[0]]) and not tied.matches([A, None, A[1]]) and not tied.matches([A, None, B])
    other = torch.zeros(4, 8)
    assert tied.matches([other, None, other[0]]) and not tied.matches([other, None, A[0]])
    # every overlapping pair is named, whichever comes first, and an empty or absent input holds no byte
    assert ops._overlaps([100, 0, 100, 96], [32, 0, 32, 8]) == ((0, 2, 0), (0, 3, -4), (2, 3, -4))
    assert ops._overlaps([100, 100, 0], [32, 0, 32]) == ()
    assert ops._overlaps([100, 132, 164], [32, 32, 32]) == ()          # side by side is apart
    assert ops._overlaps([100, 131], [32, 32]) == ((0, 1, 31),)


# ---------------------------------------------------------------------------------- hole 3: hints
@pytest.fixture
def hints(monkeypatch):
    monkeypatch.setattr(ops, "_AMAX_HINTS", {})
    monkeypatch.setattr(ops, "_check_amax", lambda name, t, device: None)         # the buffers of this tier live on the host
    return ops._AMAX_HINTS


def _hinted_conv():
    torch.manual_seed(0)
    conv = RGCNConv(8, 8, 3)
    bufs = {}
    for name, p in conv.named_parameters():
        bufs[name] = torch.zeros(ops.AMAX_FLOATS)
        ops.set_amax_hint(p, bufs[name])
        assert ops.amax_hint(p) is bufs[name]
    return conv, bufs


def test_reset_parameters_loses_every_hint(hints):
    conv, bufs = _hinted_conv()
    conv.reset_parameters()
    assert [ops.amax_hint(p) for p in conv.parameters()] == [None] * 3


def test_reset_parameters_of_a_basis_layer_loses_every_hint(hints):
    torch.manual_seed(0)
    conv = RGCNConv(8, 8, 3, num_bases=2)
    for p in conv.parameters():
        ops.set_amax_hint(p, torch.zeros(ops.AMAX_FLOATS))
    conv.reset_parameters()
    assert [ops.amax_hint(p) for p in conv.parameters()] == [None] * 4


@pytest.mark.parametrize("how", ["data_assigned", "no_grad_inplace", "detach_inplace", "withdrawn"])
def test_a_rewritten_tensor_loses_its_hint(hints, how):
    conv, bufs = _hinted_conv()
    p = conv.weight
    if how == "data_assigned":
        p.data = torch.ones_like(p)
    elif how == "no_grad_inplace":
        with torch.no_grad():
            p.mul_(2.0)
    elif how == "detach_inplace":
        p.detach().mul_(2.0)
    else:                                       # the one write nobody can see - p.data.mul_(2) - is the caller's to report
        v = p._version
        p.data.mul_(2.0)
        assert p._version == v and ops.amax_hint(p) is bufs["weight"]
        ops.set_amax_hint(p, None)
    assert ops.amax_hint(p) is None
    assert ops.amax_hint(conv.root) is bufs["root"]                    # the others keep theirs
    assert conv_mod._encoder_hints(torch.zeros(4, 8), conv, conv) is None


def test_the_hint_of_a_dead_tensor_is_never_served_to_its_successor(hints):
    t, buf = torch.zeros(4), torch.zeros(ops.AMAX_FLOATS)
    ops.set_amax_hint(t, buf)
    key, entry = id(t), hints[id(t)]
    del t
    assert key not in hints and entry[0]() is None                     # gone with its tensor
    u = torch.zeros(4)
    hints[id(u)] = entry                                               # as if u had been given the dead tensor's id
    assert ops.amax_hint(u) is None
    # and the late death of an old tensor does not take the hint of the tensor that now has its key
    ops.set_amax_hint(u, buf)
    ops._drop_amax_hint(id(u), entry[0])
    assert ops.amax_hint(u) is buf


def test_reset_parameters_draws_the_bits_it_always_drew():
    """written under ``no_grad`` instead of through ``.data``: same generator consumption, same bits"""
    torch.manual_seed(7)
    conv = RGCNConv(8, 16, 3, num_bases=2)
    with torch.no_grad():
        conv.bias.fill_(1.0)
    versions = [p._version for p in conv.parameters()]
    torch.manual_seed(11)
    conv.reset_parameters()
    got = {k: p.detach().clone() for k, p in conv.named_parameters()}
    assert all(p._version > v for p, v in zip(conv.parameters(), versions)), "a parameter was written behind its version"
    after = torch.rand(3)
    torch.manual_seed(11)
    for t in (conv.weight, conv.comp, conv.root):                      # the parent commit's reset_parameters
        bound = math.sqrt(6.0 / (t.size(-2) + t.size(-1)))
        t.data.uniform_(-bound, bound)
    conv.bias.data.zero_()
    assert sorted(got) == ["bias", "comp", "root", "weight"]
    for k, p in conv.named_parameters():
        assert torch.equal(got[k], p.detach()), k
    assert torch.equal(after, torch.rand(3)) and not conv.bias.any()


# ---------------------------------------------------------------------------------- out of memory
def test_a_replay_that_runs_out_of_memory_disables_the_plan_and_returns_the_eager_result():
    region = ops.Region("test.oom", lambda x: (x + 1,))
    owner = types.SimpleNamespace()
    plan = _plant(owner, region, plan=_StubPlan(error=torch.cuda.OutOfMemoryError("arena")))
    x = torch.arange(4.0)
    out = region.run(owner, "k", (x,), {})
    assert plan.calls == 1 and torch.equal(out[0], x + 1)
    full_key = ("test.oom", "k", ops.GEMM_PRECISION)
    assert owner._regions[full_key] == ops.Region.DISABLED
    for _ in range(3):                                                  # and it stays there: nothing is recorded again
        assert torch.equal(region.run(owner, "k", (x,), {})[0], x + 1)
        assert owner._regions == {full_key: ops.Region.DISABLED} and plan.calls == 1


def test_any_other_error_of_a_replay_reaches_the_caller():
    region = ops.Region("test.err", lambda x: (x + 1,))
    owner = types.SimpleNamespace()
    plan = _plant(owner, region, plan=_StubPlan(error=RuntimeError("rgcn_sequence_run: invalid argument")))
    with pytest.raises(RuntimeError, match="rgcn_sequence_run"):
        region.run(owner, "k", (torch.arange(4.0),), {})
    assert owner._regions[("test.err", "k", ops.GEMM_PRECISION)] is plan


# ---------------------------------------------------------------------------------- hole 5: edge dropout after its parent
def test_an_edge_dropout_refuses_to_work_on_a_destroyed_parent_before_any_library_call(monkeypatch):
    def library_call():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(ops._lib, "load", library_call)
    monkeypatch.setattr(ops, "_L", library_call)
    parent = _graph()
    ed = ops.EdgeDropout.__new__(ops.EdgeDropout)
    view = ops._EdgeDropoutView.__new__(ops._EdgeDropoutView)
    try:
        ed._handle, ed.graph, ed.device = ctypes.c_void_p(FAKE + 8), parent, parent.device
        view._handle, view.parent, view.device = ctypes.c_void_p(FAKE + 16), parent, parent.device
        view.bipartite, view.weighted_shard, view.num_relations = False, True, 3
        ed.view = view
        assert ed.handle.value == FAKE + 8 and view.handle.value == FAKE + 16                    # the parent lives
        plan = _plant(view)
        assert REGION.run(view, "k", (torch.zeros(4, 8),), dict(graph=view)) == ["replayed"]
        parent._handle = None                                           # ... and is destroyed
        rng = torch.zeros(2, dtype=torch.int64)
        with pytest.raises(RuntimeError, match="parent BucketedGraph .* was destroyed"):
            ed.draw(0.5, rng)
        with pytest.raises(RuntimeError, match="parent BucketedGraph .* was destroyed"):
            ed.draw(7.0, None)                                          # before every other complaint, too
        with pytest.raises(RuntimeError, match="parent BucketedGraph .* was destroyed"):
            ed.kept_counts()
        with pytest.raises(RuntimeError, match="parent BucketedGraph .* was destroyed"):
            view.handle
        with pytest.raises(RuntimeError, match="parent BucketedGraph .* was destroyed"):
            view.tile_mask_ptr(False)
        assert not view.alive
        with pytest.raises(RuntimeError, match="parent BucketedGraph .* was destroyed"):
            REGION.run(view, "k", (torch.zeros(4, 8),), dict(graph=view))
        assert plan.calls == 1
    finally:
        ed._handle = None                                               # a fake handle must never reach the library
