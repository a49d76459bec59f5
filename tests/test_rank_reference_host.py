"""The host restatement of the ranking count (``rank_reference.py``), the part that needs no GPU: against a brute-force
python loop with NaN and infinities everywhere, against the ``>`` form the finite tests use, and against the
reference protocol's argsort."""
import itertools

import torch

from rank_reference import brute_rank, eligible_mask, restate_rank
from test_rank_filter import _host_rank

NAN, INF = float("nan"), float("inf")


def _tiny(seed, b=9, n=23):
    g = torch.Generator().manual_seed(seed)
    s = torch.randn(b, n, generator=g)
    target = torch.randint(0, n, (b,), generator=g)
    allowed = torch.rand(b, n, generator=g) < 0.6
    known = torch.rand(b, n, generator=g) < 0.3
    return s, target, allowed, known


def test_restatement_against_a_brute_force_loop_with_every_non_finite_value():
    s, target, allowed, known = _tiny(3)
    b, n = s.shape
    s[0, 2], s[0, 5], s[0, 7] = NAN, INF, -INF
    s[1] = NAN                                                   # a NaN score row (a NaN query)
    s[2, :4] = torch.tensor([INF, INF, -INF, -INF])
    s[3, 4], s[3, 9] = NAN, NAN
    s[4, 1] = s[4, 0]                                            # a finite tie
    allowed[5] = False                                           # a row without an eligible candidate
    known[6] = True
    poisons = (None, NAN, INF, -INF)
    for a, e in itertools.product((None, allowed), (None, known)):
        for kind in poisons:
            for tgt in (target, torch.full((b,), -1), torch.full((b,), n), torch.where(torch.arange(b) % 2 == 0, target, -5)):
                true = s.gather(1, tgt.clamp(0, n - 1).view(-1, 1)).view(-1).clone()
                if kind is not None:
                    true[::2] = kind
                got, want = restate_rank(s, true, tgt, a, e), brute_rank(s, true, tgt, a, e)
                assert torch.equal(got, want), (a is None, e is None, kind, tgt.tolist())
                elig = eligible_mask(tgt, s.shape, a, e).sum(1)
                nan_true = torch.isnan(true)
                # a NaN true score is beaten by every eligible candidate (torch's descending argsort would put the
                # NaN entry FIRST, or anywhere among other NaN scores: rank 1 for a missing value)
                assert torch.equal(got[nan_true], 1 + elig[nan_true])
                assert bool((got >= 1).all()) and bool((got <= 1 + elig).all())
    # equal scores do not count, infinities included; a NaN candidate counts against every true score
    row = torch.tensor([[0.5, NAN, 2.0, -INF, INF, NAN, 1.0, INF, -INF]])
    none = torch.tensor([-1])
    for true, want in ((2.0, 5), (INF, 3), (-INF, 8), (NAN, 10), (0.5, 7)):
        assert restate_rank(row, torch.tensor([true]), none).tolist() == [want] == brute_rank(row, torch.tensor([true]), none).tolist()
    assert restate_rank(row, torch.tensor([INF]), torch.tensor([4])).tolist() == [3]      # +inf against the other +inf: no count
    assert restate_rank(row, torch.tensor([-INF]), torch.tensor([3])).tolist() == [8]     # -inf against the other -inf: no count
    assert restate_rank(row, torch.tensor([NAN]), torch.tensor([1])).tolist() == [9]      # 1 + the eight other candidates
    # a target outside [0, N) strikes nothing
    assert eligible_mask(torch.tensor([-1, 9, 3]), (3, 9)).sum(1).tolist() == [9, 9, 8]


def test_on_finite_data_it_is_the_greater_than_form():
    for seed in range(4):
        s, target, allowed, known = _tiny(10 + seed, b=17, n=70)
        s[0, 3] = s[0, int(target[0])]                           # a tie with the true score: does not count in either form
        true = s.gather(1, target.view(-1, 1)).view(-1)
        for a, e in itertools.product((None, allowed), (None, known)):
            assert torch.equal(restate_rank(s, true, target, a, e), _host_rank(s, true, target, a, e))
        off = true + 0.25                                        # a true score that is no entry of the row
        assert torch.equal(restate_rank(s, off, target), _host_rank(s, off, target))


def test_with_a_finite_untied_true_score_it_is_the_reference_protocols_argsort():
    """``evaluate.py:266-274`` of the reference: the position of the true tail in ``argsort(scores, descending=True)``.
    torch orders NaN above every number, so a NaN candidate counts there as it does here."""
    g = torch.Generator().manual_seed(21)
    s = torch.randn(40, 57, generator=g)
    target = torch.randint(0, 57, (40,), generator=g)
    for r in range(40):                                          # NaN, +inf, -inf candidates, never on the target
        for j, v in enumerate((NAN, INF, -INF, NAN, INF)):
            if r % (j + 2) == 0:
                c = (int(target[r]) + 1 + 3 * j + r) % 57
                if c != int(target[r]):
                    s[r, c] = v
    assert bool(torch.isnan(s).any()) and bool((s == INF).any()) and bool((s == -INF).any())
    true = s.gather(1, target.view(-1, 1)).view(-1)
    assert bool(torch.isfinite(true).all()) and bool(((s == true[:, None]).sum(1) == 1).all())   # finite, untied
    want = torch.tensor([int((torch.argsort(s[i], descending=True) == target[i]).nonzero()) + 1 for i in range(40)])
    assert torch.equal(restate_rank(s, true, target), want)
    assert not torch.equal(_host_rank(s, true, target), want)    # the > form ranks a NaN candidate below the true entry
    # one row by hand: argsort ranks the 2.0 fourth (inf and both NaN above it), the > form second
    row = torch.tensor([[0.5, NAN, 2.0, -INF, INF, NAN, 1.0]])
    assert int((torch.argsort(row[0], descending=True) == 2).nonzero()) + 1 == 4
    assert restate_rank(row, torch.tensor([2.0]), torch.tensor([2])).tolist() == [4]
    assert _host_rank(row, torch.tensor([2.0]), torch.tensor([2])).tolist() == [2]


def test_a_nan_true_score_ranks_last_among_the_eligible():
    s, target, allowed, known = _tiny(5, b=12, n=33)
    s[3, 4] = NAN
    true = torch.full((12,), NAN)
    assert restate_rank(s, true, target).tolist() == [33] * 12                       # raw: N
    for a, e in itertools.product((None, allowed), (None, known)):
        want = 1 + eligible_mask(target, s.shape, a, e).sum(1)
        assert torch.equal(restate_rank(s, true, target, a, e), want)
    # torch gives something else: its descending argsort puts NaN first, so a row whose only NaN is the true entry
    # would get rank 1 from the reference protocol - a metric that improves because a value is missing
    row = torch.tensor([1.0, NAN, 3.0])
    assert int((torch.argsort(row, descending=True) == 1).nonzero()) + 1 == 1
    assert restate_rank(row.view(1, -1), torch.tensor([NAN]), torch.tensor([1])).tolist() == [3]
