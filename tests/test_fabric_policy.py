"""The queue fabric's two policies as pure functions (csrc/fabric_policy.h): which consumer gets a
produced frame, and how a consumer deals its free slots to its producers.  QueueFabric's passes
call exactly these; here they are called with numbers -- no threads, no rings, no GPU.

Policies: 0 balanced, 1 local_first, 2 spread.  kLocalSlack = 64, kFeedLocalReady = 2, kMinGrants = 4.
"""
import pytest


def route(native, policy, n_offers, cands, local_credit, n_ready=0, rr=0):
    """cands: (avail, keeper, may_starve) per remote link.  Offers are numbered 0 .. n_offers-1."""
    local, assign, left, rr, credit = native.fabric_route(
        policy, list(range(n_offers)), [c[0] for c in cands], [c[1] for c in cands], [c[2] for c in cands],
        local_credit, n_ready, rr)
    # every offer ends in exactly one place, in FIFO order within it
    assert sorted(local + [s for a in assign for s in a] + left) == list(range(n_offers))
    assert credit == local_credit - len(local)
    return local, assign, left, rr


REAL, KEEPER, STARVING = (False, False), (True, False), (False, True)


def test_local_first_uses_local_credit_then_the_remote(native):
    local, assign, left, _ = route(native, 1, 5, [(100, *REAL)], local_credit=3)
    assert (local, assign, left) == ([0, 1, 2], [[3, 4]], [])


def test_balanced_stays_local_within_the_slack(native):
    """Local wins while local_credit + kLocalSlack >= the remote's remaining grants."""
    local, assign, left, _ = route(native, 0, 4, [(74, *REAL)], local_credit=10, n_ready=0)
    assert (local, assign, left) == ([0, 2], [[1, 3]], [])


def test_keeper_is_the_last_resort(native):
    local, assign, left, _ = route(native, 0, 3, [(5, *KEEPER), (1, *REAL)], local_credit=0)
    assert (local, assign, left) == ([], [[1, 2], [0]], [])


def test_spread_goes_round_every_consumer_with_credit(native):
    local, assign, left, rr = route(native, 2, 5, [(5, *REAL), (5, *REAL)], local_credit=5, rr=0)
    assert (local, assign, left, rr) == ([2], [[0, 3], [1, 4]], [], 2)


def test_balanced_feeds_a_starving_pair_once_the_own_consumer_is_fed(native):
    local, assign, left, _ = route(native, 0, 4, [(3, *STARVING), (3, *STARVING)], local_credit=4, n_ready=2)
    assert (local, assign, left) == ([], [[0, 2], [1, 3]], [])


def test_balanced_feeds_nobody_ahead_of_a_hungry_own_consumer(native):
    """Fewer than kFeedLocalReady frames ready at the own consumer: it comes first."""
    local, assign, left, _ = route(native, 0, 4, [(3, *STARVING), (3, *STARVING)], local_credit=4, n_ready=1)
    assert (local, assign, left) == ([0, 1, 2, 3], [[], []], [])


def test_no_credit_anywhere_routes_nothing(native):
    local, assign, left, _ = route(native, 0, 3, [(0, *REAL)], local_credit=0)
    assert (local, assign, left) == ([], [[]], [0, 1, 2])


def test_grants_scarce_free_slots_are_dealt_round_robin(native):
    want, total, _ = native.fabric_grant_shares(32, [0, 100], [0, 0])
    assert (want, total) == ([8, 32], 32)
    _, _, share = native.fabric_grant_shares(32, [0, 100], [0, 0], free_slots=20)
    assert share == [8, 12]


def test_grants_are_bound_by_the_prefetch(native):
    want, total, share = native.fabric_grant_shares(32, [0, 100], [0, 0], prefetch=10, held=4)
    assert (want, total, share) == ([8, 32], 6, [3, 3])


def test_grants_minimum_at_an_idle_producer(native):
    want, total, share = native.fabric_grant_shares(6, [0], [0])
    assert (want, total, share) == ([4], 4, [4])


def test_route_rejects_mismatched_candidate_lists(native):
    with pytest.raises(RuntimeError):
        native.fabric_route(0, [0], [1, 2], [False], [False, False], 0, 0, 0)
