"""CPU tier of the constrained batch sampler (``csrc/sampler_constrained.hip``, ``include/rgcn_sampling.h``): the
C surface, the argument checks that run before any launch, ``ops.NodeClasses``, the trainer's flags - and the host
restatement of the sampler's contract that ``test_sampler_constrained.py`` holds the device to, bit for bit.

The contract, from its words:

* Positives, relations, labels, the clamping of a window past the end and ``ctr = (cursor + p) * k + j`` are exactly
  the plain sampler's.
* Block t, t = 0 .. T-1, is Philox4x32-10 with key = the two halves of the seed and counter
  ``(ctr_lo, ctr_hi, epoch_lo, epoch_hi XOR (t << 24))``; block 0 is the plain sampler's block; epochs stay below 2^56.
* Side: the top bit of word 0 of block 0.  Set: the head is replaced, the anchor is the tail, the known side is
  ``"head"``.  Clear: the tail is replaced, the anchor is the head, the known side is ``"tail"``.
* Candidate of try t, w = word 1 of block t.  No classes: ``(w * N) >> 32``.  With classes, c = ``class_of[replaced
  node]``: c < 0 or class c empty -> ``(w * N) >> 32``, otherwise ``class_members[class_ptr[c] + ((w * size_c) >> 32)]``
  (members ascending within a class).
* The first accepted candidate wins; accepted = no known set given, or ``(anchor, relation, candidate)`` not in it.
  Every rejected draw adds 1 to ``stats[0]``.
* All T draws rejected: the last candidate is kept and ``stats[1]`` gains 1.
* All three groups null and T = 1: the output of ``rgcn_sample_batch``, bit for bit.

The host Philox is pinned to the published Random123 known-answer vectors first.
"""
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
from primekg_rgcn_linkprediction_amd import _lib, ops, train as T

M32 = 0xFFFFFFFF
M64 = 0xFFFFFFFFFFFFFFFF

SEED = 0x1234_5678_9ABC_DEF0             # both halves of the key matter
EPOCH = (1 << 33) + 5                    # so do both epoch words of the counter


# ---------------------------------------------------------------------------------- the restatement
def philox4x32_10(ctr, key):
    """Philox4x32 with ten rounds (Salmon et al., SC'11) on Python ints: ctr 4 words, key 2 words -> 4 words"""
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def host_batch(ei, et, order, cursor, batch, k, num_nodes, seed, epoch):
    """the PLAIN sampler's contract: (heads, tails, rels int64 [B(1+k)], labels f32) - positives ``order[cursor :
    cursor + B]`` (a window over the end repeats the last column), then the k corruptions of each positive"""
    e = ei.shape[1]
    total = batch * (1 + k)
    heads, tails, rels = (np.empty(total, dtype=np.int64) for _ in range(3))
    key = (seed & M32, (seed >> 32) & M32)
    for p in range(batch):
        pos = min(max(cursor + p, 0), e - 1)
        col = int(order[pos]) if order is not None else pos
        col = min(max(col, 0), e - 1)
        h, t, r = int(ei[0, col]), int(ei[1, col]), int(et[col])
        heads[p], tails[p], rels[p] = h, t, r
        for j in range(k):
            ctr = ((cursor + p) * k + j) & M64
            w = philox4x32_10((ctr & M32, ctr >> 32, epoch & M32, (epoch >> 32) & M32), key)
            entity = (w[1] * num_nodes) >> 32
            i = batch + p * k + j
            heads[i], tails[i], rels[i] = (entity, t, r) if w[0] >> 31 else (h, entity, r)
    labels = np.concatenate([np.ones(batch, dtype=np.float32), np.zeros(batch * k, dtype=np.float32)])
    return heads, tails, rels, labels


def known_sets(ei, et):
    """side -> {(anchor, relation, other)} of a graph's columns: what ``KnownTriples.csr(side)`` indexes"""
    h, t, r = (np.asarray(v).tolist() for v in (ei[0], ei[1], et))
    return {"tail": set(zip(h, r, t)), "head": set(zip(t, r, h))}


def host_batch_constrained(ei, et, order, cursor, batch, k, num_nodes, seed, epoch, tries, class_of=None, known=None):
    """the CONSTRAINED sampler's contract -> (heads, tails, rels, labels, (rejected draws, gave up)).  ``class_of``:
    one int per node, negative = no class; ``known``: ``known_sets`` of the graph to filter against"""
    assert epoch < 1 << 56 and 1 <= tries <= 16
    e = ei.shape[1]
    total = batch * (1 + k)
    heads, tails, rels = (np.empty(total, dtype=np.int64) for _ in range(3))
    key = (seed & M32, (seed >> 32) & M32)
    members = {}
    if class_of is not None:
        for node, c in enumerate(np.asarray(class_of).tolist()):        # node ids ascending within each class
            if c >= 0:
                members.setdefault(c, []).append(node)
    rejected = gave_up = 0
    for p in range(batch):
        pos = min(max(cursor + p, 0), e - 1)
        col = int(order[pos]) if order is not None else pos
        col = min(max(col, 0), e - 1)
        h, t, r = int(ei[0, col]), int(ei[1, col]), int(et[col])
        heads[p], tails[p], rels[p] = h, t, r
        for j in range(k):
            ctr = ((cursor + p) * k + j) & M64
            block = lambda tr: philox4x32_10((ctr & M32, ctr >> 32, epoch & M32, ((epoch >> 32) & M32) ^ (tr << 24)), key)  # noqa: E731
            replace_head = bool(block(0)[0] >> 31)
            replaced, anchor, side = (h, t, "head") if replace_head else (t, h, "tail")
            pool = members.get(int(class_of[replaced]), []) if class_of is not None else []
            for tr in range(tries):
                w = block(tr)[1]
                cand = pool[(w * len(pool)) >> 32] if pool else (w * num_nodes) >> 32
                if known is None or (anchor, r, cand) not in known[side]:
                    break
                rejected += 1
                gave_up += tr + 1 == tries
            i = batch + p * k + j
            heads[i], tails[i], rels[i] = (cand, t, r) if replace_head else (h, cand, r)
    labels = np.concatenate([np.ones(batch, dtype=np.float32), np.zeros(batch * k, dtype=np.float32)])
    return heads, tails, rels, labels, (rejected, gave_up)


# what the GPU tier runs, defined here so that the conditions it rests on are checked without a GPU
GRID = [(64, 5000, 257, 3, 4), (7, 40, 33, 1, 1), (7, 40, 33, 1, 16), (1000, 5000, 64, 2, 8)]   # N, E, batch, k, T
NUM_RELATIONS = 4
SMALL_CLASSES = [2, -1, 1, 2, -1, 2, 2]      # N = 7: class 0 is empty, class 1 has one member (node 2), two nodes have none
SPARSE = (1000, 5000, 512, 2, 16)            # N, E, batch, k, T of the property and batch-split tests


def make_graph(n, e, seed):
    gen = torch.Generator().manual_seed(seed)
    ei = torch.randint(0, n, (2, e), generator=gen)
    et = torch.randint(0, NUM_RELATIONS, (e,), generator=gen)
    order = torch.randperm(e, generator=gen)
    if n == 7:                               # the column a window past the end repeats joins the single-member class's node
        ei[:, order[-1]] = SMALL_CLASSES.index(1)
    return ei, et, order


def make_classes(n, seed=5):
    """three classes; on the 7-node graph an empty one, a single-member one and nodes without a class"""
    if n == 7:
        return torch.tensor(SMALL_CLASSES, dtype=torch.int32)
    gen = torch.Generator().manual_seed(seed)
    return torch.randint(-1, 3, (n,), generator=gen).to(torch.int32)


def restate(ei, et, order, cursor, batch, k, n, tries, class_of=None, known=None, seed=SEED, epoch=EPOCH):
    """``host_batch_constrained`` of the tensors the device call takes"""
    return host_batch_constrained(ei.numpy(), et.numpy(), None if order is None else order.numpy(), cursor, batch, k, n,
                                  seed, epoch, tries, None if class_of is None else class_of.numpy(), known)


def test_host_philox_reproduces_the_published_vectors():
    """Random123's kat_vectors for philox4x32 10: zeros, all ones, and the digits of pi"""
    f = M32
    assert philox4x32_10((0, 0, 0, 0), (0, 0)) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)
    assert philox4x32_10((f, f, f, f), (f, f)) == (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)
    assert philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0)) == \
        (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)


@pytest.mark.parametrize("n,e,batch,k,tries", GRID)
@pytest.mark.parametrize("cursor", [0, 1031])
def test_restatement_without_groups_is_the_plain_contract(n, e, batch, k, tries, cursor):
    """no classes, no known set: nothing is ever rejected, so every T gives block 0's draw - the plain sampler's"""
    ei, et, order = make_graph(n, e, 11)
    *got, stats = restate(ei, et, order, cursor, batch, k, n, tries)
    want = host_batch(ei.numpy(), et.numpy(), order.numpy(), cursor, batch, k, n, SEED, EPOCH)
    assert stats == (0, 0)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w)


def test_restatement_meets_the_conditions_the_gpu_tier_rests_on():
    """the 7-node graph's single-member class gives up (its only candidate is the known positive itself) for T = 1 and
    T = 16; the sparse graph with T = 16 never does; the tries beyond the first really change draws"""
    ei, et, order = make_graph(7, 40, 11)
    for tries in (1, 16):
        for cursor in (0, 1031):
            *_, stats = restate(ei, et, order, cursor, 33, 1, 7, tries, make_classes(7), known_sets(ei, et))
            assert stats[1] > 0 and stats[0] >= stats[1] * tries
    assert stats == (33 * 16, 33)            # past the end every positive is (2, r, 2): each of the 16 draws is node 2 again
    n, e, batch, k, tries = SPARSE
    ei, et, order = make_graph(n, e, 12)
    cls, known = make_classes(n), known_sets(ei, et)
    h, t, r, _, stats = restate(ei, et, order, 0, batch, k, n, tries, cls, known)
    assert stats[1] == 0 and stats[0] > 0
    h1, t1, *_ = restate(ei, et, order, 0, batch, k, n, 1, cls, known)
    assert not (np.array_equal(h, h1) and np.array_equal(t, t1))
    # the properties themselves, on the host: class kept, nothing known
    ph, pt = np.repeat(h[:batch], k), np.repeat(t[:batch], k)
    nh, nt, nr = h[batch:], t[batch:], r[batch:]
    c = cls.numpy()
    head_replaced = nt == pt
    replaced, new = np.where(head_replaced, ph, pt), np.where(head_replaced, nh, nt)
    assert bool(((c[replaced] < 0) | (c[new] == c[replaced])).all())
    assert not any((a, b, d) in known["tail"] for a, b, d in zip(nh.tolist(), nr.tolist(), nt.tolist()))


# ---------------------------------------------------------------------------------- C surface
def _call(lib, batch=0, num_neg=1, num_nodes=100, tries=8, classes=(None, None, None, 0),
          known=(None, None, None, 0, 0, None, None, None, 0, 0, 0)):
    """the entry point with NULL graph arrays and outputs, so that no case can reach a launch: with a batch it is
    refused at the latest for those, and with ``batch=0`` - where a call that passes every check returns RGCN_OK -
    the code tells which check spoke.  The group pointers are fakes that are never dereferenced."""
    return lib.rgcn_sample_batch_constrained(None, None, 10, None, None, batch, num_neg, num_nodes, None, *classes, *known,
                                             tries, None, None, None, None, None, None)


def test_return_codes_without_a_gpu():
    """every refusal comes before any launch: nulls, T outside 1..16, half-given groups; an empty batch is OK"""
    lib = _lib.load()
    A, U, OK = _lib.RGCN_ERR_ARG, _lib.RGCN_ERR_UNSUPPORTED, _lib.RGCN_OK
    assert _call(lib, batch=4) == A and _call(lib, batch=4, num_neg=0) == A       # null graph arrays and outputs
    assert _call(lib, num_nodes=0) == A and _call(lib, batch=-1) == A and _call(lib, num_neg=-1) == A
    for tries in (0, 17, -1):
        assert _call(lib, tries=tries) == A and _call(lib, batch=4, tries=tries) == A
    assert _call(lib) == OK and _call(lib, tries=1) == OK and _call(lib, tries=16) == OK
    assert _call(lib, num_nodes=1 << 32) == OK and _call(lib, num_nodes=(1 << 32) + 1) == U
    # half-given groups
    for classes in ((256, None, None, 3), (256, 256, None, 3), (None, 256, 256, 3), (256, None, 256, 3), (256, 256, 256, 0)):
        assert _call(lib, classes=classes) == A, classes                          # e.g. class_of without class_ptr
    full = [256, 256, 256, 5, 9, 256, 256, 256, 5, 9, 3]
    for hole in (0, 1, 2, 5, 6, 7):
        known = list(full)
        known[hole] = None
        assert _call(lib, known=tuple(known)) == A, hole                          # e.g. keys without ids
    assert _call(lib, known=(256, 256, 256, 5, 9, None, None, None, 0, 0, 3)) == A   # one side only
    for zero in (3, 4, 8, 9, 10):
        known = list(full)
        known[zero] = 0
        assert _call(lib, known=tuple(known)) == A, zero                          # a given group that holds nothing
    assert _call(lib, classes=(256, 256, 256, 3), known=tuple(full)) == OK
    assert _call(lib, batch=4, classes=(256, 256, 256, 3), known=tuple(full)) == A   # whole groups, still no graph


def test_sorted_search_is_exact_and_clean_under_sanitizers(tmp_path):
    """``tests/sampler_search_check.cpp``: the kernel's own search (``csrc/rgcn_sorted_search.h``) against
    ``std::lower_bound`` on exactly sized arrays, stand-alone under AddressSanitizer and UndefinedBehaviorSanitizer
    (their runtimes are linked INTO the program, so it runs as it is, whatever the loader's environment)"""
    import shutil
    import subprocess
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path / "sampler_search_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", ROOT,
                    os.path.join(ROOT, "tests", "sampler_search_check.cpp"), "-o", str(exe)], check=True)
    done = subprocess.run([str(exe)], capture_output=True, text=True)
    assert done.returncode == 0 and done.stdout.startswith("sampler_search_check ok"), done.stdout + done.stderr


# ---------------------------------------------------------------------------------- ops.NodeClasses
def test_node_classes_on_cpu_tensors():
    nc = ops.NodeClasses(torch.tensor(SMALL_CLASSES), 3)                         # empty class 0, single-member class 1, two -1
    assert nc.class_of.dtype == torch.int32 and nc.class_of.tolist() == SMALL_CLASSES
    assert nc.ptr.dtype == nc.members.dtype == nc.sizes.dtype == torch.int64
    assert nc.sizes.tolist() == [0, 1, 4] and nc.ptr.tolist() == [0, 0, 1, 5]
    assert nc.members.tolist() == [2, 0, 3, 5, 6]                               # ascending within each class
    assert (nc.num_nodes, nc.num_classes) == (7, 3)
    gen = torch.Generator().manual_seed(0)
    class_of = torch.randint(-1, 5, (1000,), generator=gen).to(torch.int32)
    nc = ops.NodeClasses(class_of, 6)                                            # class 5 exists and is empty
    assert nc.sizes.tolist() == [int((class_of == c).sum()) for c in range(6)] and nc.sizes[5] == 0
    for c in range(6):
        assert nc.members[nc.ptr[c]: nc.ptr[c + 1]].tolist() == (class_of == c).nonzero().flatten().tolist()
    assert int(nc.ptr[-1]) == int((class_of >= 0).sum()) == nc.members.numel()
    none = ops.NodeClasses(torch.full((5,), -1), 2)
    assert none.members.numel() == 0 and none.ptr.tolist() == [0, 0, 0]
    with pytest.raises(IndexError):
        ops.NodeClasses(torch.tensor([0, 3, 1]), 3)
    with pytest.raises(ValueError):
        ops.NodeClasses(torch.zeros(0, dtype=torch.int32), 3)
    with pytest.raises(ValueError):
        ops.NodeClasses(torch.zeros((2, 2), dtype=torch.int32), 3)
    with pytest.raises(ValueError):
        ops.NodeClasses(torch.tensor([0, 1]), 0)


def test_sample_batch_constrained_refuses_cpu_tensors():
    ei, et, _ = make_graph(7, 40, 11)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.sample_batch_constrained(ei, et, None, None, 4, 0, 7, None)


# ---------------------------------------------------------------------------------- trainer flags
def test_parser_flags_and_defaults():
    a = T.parse_args([])
    assert (a.filtered_negatives, a.type_constrained_negatives, a.node_types, a.negative_tries) == (False, False, None, 8)
    a = T.parse_args(["--filtered_negatives", "--type_constrained_negatives", "--node_types", "types.npz",
                      "--negative_tries", "3"])
    assert (a.filtered_negatives, a.type_constrained_negatives, a.node_types, a.negative_tries) == (True, True, "types.npz", 3)
    assert T.VALIDATION_STREAM < 1 << 56


def _tiny_trainer(tmp_path, device, **flags):
    gen = torch.Generator().manual_seed(0)
    data = {"edge_index": torch.randint(0, 20, (2, 60), generator=gen), "edge_type": torch.randint(0, 3, (60,), generator=gen),
            "num_nodes": 20, "num_relations": 3}
    args = T.parse_args(["--output_dir", str(tmp_path), "--embedding_dim", "16", "--hidden_dim", "32", "--batch_size", "16"])
    for k, v in flags.items():
        setattr(args, k, v)
    return T.Trainer(T.create_model(20, 3, args), data, data, data, torch.device(device), args)


def test_constraint_flag_combinations_are_refused_at_construction(tmp_path):
    types = tmp_path / "types.npz"
    np.savez(types, node_class=(np.arange(20) % 3).astype(np.int32))
    for flags in ({"filtered_negatives": True}, {"type_constrained_negatives": True, "node_types": str(types)}):
        with pytest.raises(ValueError, match="torch_sampler"):
            _tiny_trainer(tmp_path, "cuda", torch_sampler=True, **flags)
        with pytest.raises(ValueError, match="GPU only"):
            _tiny_trainer(tmp_path, "cpu", **flags)
    with pytest.raises(ValueError, match="node_types"):
        _tiny_trainer(tmp_path, "cuda", type_constrained_negatives=True)
    with pytest.raises(ValueError, match="negative_tries"):
        _tiny_trainer(tmp_path, "cuda", filtered_negatives=True, negative_tries=17)
    trainer = _tiny_trainer(tmp_path, "cpu")                                   # the defaults still construct on the CPU
    assert not trainer.constrained_negatives and trainer._neg_stats is None
