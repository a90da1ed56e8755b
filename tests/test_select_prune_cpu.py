"""CPU: the host selection of mrgfe_batch_align_best (mrgfe_dbg_select_prune) against the reference's best-candidate rule
(loop_detector.cpp:126-145, loop_closure.select_best).  Random certified intervals go in, an exact score is drawn inside each, and the records
the product would return (exact score, or the lower bound where it pruned / capped, DBL_MAX where it skipped) must give the rule's winner and
score on the exact values — per group and for unions of groups; with a cap, the same or "above the cap" exactly where the exact best is."""
import ctypes as C
import os

import numpy as np
import pytest

os.environ.setdefault("MRGFE_NO_TORCH", "1")

from mrg_slam_amd import _lib  # noqa: E402
from mrg_slam_amd.loop_closure import select_best  # noqa: E402
from mrg_slam_amd.registration import RESULT_DTYPE  # noqa: E402

BIG = np.finfo(np.float64).max
_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)


def prune(lower, upper, converged, group, n_groups, cap=BIG):
    n = len(lower)
    lo = np.ascontiguousarray(lower, dtype=np.float64)
    hi = np.ascontiguousarray(upper, dtype=np.float64)
    cv = np.ascontiguousarray(converged, dtype=np.int32)
    gr = np.ascontiguousarray(group, dtype=np.int32)
    st = np.full(max(n, 1), -7, dtype=np.int32)
    rc = _lib.lib().mrgfe_dbg_select_prune(n, lo.ctypes.data_as(_dp), hi.ctypes.data_as(_dp), cv.ctypes.data_as(_ip), gr.ctypes.data_as(_ip), n_groups, cap,
                                           st.ctypes.data_as(_ip))
    assert rc == 0, _lib.lib().mrgfe_last_error()
    return st[:n]


def records(values, converged):
    r = np.zeros(len(values), dtype=RESULT_DTYPE)
    r["fitness"] = values
    r["converged"] = converged
    return r


def stored(state, exact, lower):
    """what align_best leaves in the fitness field"""
    return np.where(state == _lib.FIT_EXACT, exact, np.where(state == _lib.FIT_SKIPPED, BIG, lower))


def same(a, b):
    (ia, sa), (ib, sb) = a, b
    return ia == ib and (sa == sb or (np.isnan(sa) and np.isnan(sb)))


SPECIAL = [BIG, np.inf, np.nan]


def draw_case(rng, n, n_groups):
    """intervals over a small value set (so ties, lower == another's upper and degenerate intervals are common), specials sprinkled in"""
    grid = np.array([0.25, 0.5, 0.75, 1.0, 1.25, 1.5, 2.0, 3.0])
    lower = np.empty(n)
    upper = np.empty(n)
    exact = np.empty(n)
    for i in range(n):
        kind = rng.random()
        if kind < 0.06:  # a special value somewhere in the interval
            sp = SPECIAL[rng.integers(3)]
            if np.isnan(sp):
                lower[i], upper[i] = (np.nan, rng.choice(grid)) if rng.random() < 0.5 else (rng.choice(grid), np.nan)
                exact[i] = np.nan if rng.random() < 0.5 else rng.choice(grid)
            else:
                lower[i] = sp if rng.random() < 0.5 else rng.choice(grid)
                upper[i] = sp
                exact[i] = sp if lower[i] == sp or rng.random() < 0.5 else lower[i]
        elif kind < 0.14:  # no certified interval
            lower[i], upper[i] = 0.0, np.inf
            exact[i] = rng.choice(grid) if rng.random() < 0.8 else BIG
        else:
            a, b = np.sort(rng.choice(grid, 2))
            if rng.random() < 0.25:
                b = a  # degenerate
            lower[i], upper[i] = a, b
            u = rng.random()
            exact[i] = a if u < 0.3 else (b if u < 0.6 else a + (b - a) * rng.random())
    converged = (rng.random(n) < 0.8).astype(np.int32)
    group = rng.integers(-1, n_groups, n).astype(np.int32)
    return lower, upper, exact, converged, group


def check_groups(lower, upper, exact, converged, group, n_groups, cap, rng):
    state = prune(lower, upper, converged, group, n_groups, cap)
    assert set(np.unique(state)) <= {0, 1, 2, 3}
    assert (state[group < 0] == _lib.FIT_EXACT).all()
    assert (state[(group >= 0) & (converged == 0)] == _lib.FIT_SKIPPED).all()
    if cap == BIG:
        assert not (state == _lib.FIT_ABOVE_CAP).any() or np.isinf(lower[state == _lib.FIT_ABOVE_CAP]).all()
    vals = stored(state, exact, lower)
    full = records(exact, converged)
    mine = records(vals, converged)
    for g in range(n_groups):
        idx = np.flatnonzero(group == g)
        if (np.isnan(lower[idx]) | np.isnan(upper[idx]))[converged[idx] != 0].any():
            assert (state[idx][converged[idx] != 0] == _lib.FIT_EXACT).all()
        # every pruned value is strictly above the exact score of a converged candidate of its group — without a cap, one that is scored exactly
        for i in idx[state[idx] == _lib.FIT_PRUNED]:
            keep = (converged[idx] != 0) & ((state[idx] == _lib.FIT_EXACT) if cap == BIG else True)
            assert (vals[i] > exact[idx][keep]).any()
        want, got = select_best(full[idx]), select_best(mine[idx])
        if cap == BIG:
            assert same(want, got), (g, want, got, lower[idx], upper[idx], exact[idx], converged[idx], state[idx])
        else:
            has = (converged[idx] != 0).any()
            if has and want[1] > cap:  # the -2 case: the records' best is above the cap too
                assert got[1] > cap, (g, want, got)
            else:
                assert same(want, got), (g, want, got, lower[idx], upper[idx], exact[idx], converged[idx], state[idx])
    # unions of groups, in pair order (a NaN score lets everything after it through: unions holding one are not compared)
    for _ in range(6):
        pick = rng.random(n_groups) < 0.5
        idx = np.flatnonzero((group >= 0) & pick[np.maximum(group, 0)])
        if np.isnan(exact[idx][converged[idx] != 0]).any() or np.isnan(vals[idx][converged[idx] != 0]).any():
            continue
        want, got = select_best(full[idx]), select_best(mine[idx])
        if cap != BIG and want[1] > cap:
            assert got[1] > cap
        else:
            assert same(want, got), (want, got)


@pytest.mark.parametrize("seed", range(40))
def test_random_intervals_keep_the_winner(seed):
    rng = np.random.default_rng(seed)
    n_groups = int(rng.integers(1, 9))
    n = int(rng.integers(1, 60))
    lower, upper, exact, converged, group = draw_case(rng, n, n_groups)
    check_groups(lower, upper, exact, converged, group, n_groups, BIG, rng)


@pytest.mark.parametrize("seed", range(40))
@pytest.mark.parametrize("cap", [1.25, 0.5, 0.0])
def test_random_intervals_with_a_cap(seed, cap):
    rng = np.random.default_rng(1000 + seed)
    n_groups = int(rng.integers(1, 9))
    n = int(rng.integers(1, 60))
    lower, upper, exact, converged, group = draw_case(rng, n, n_groups)
    check_groups(lower, upper, exact, converged, group, n_groups, cap, rng)


def test_ties_stay_contenders_and_the_last_wins():
    # b's lower bound equals a's upper bound: neither may be pruned; c is strictly above and goes
    lower = [0.5, 1.0, 1.5, 1.0]
    upper = [1.0, 2.0, 3.0, 1.0]
    st = prune(lower, upper, [1, 1, 1, 1], [0, 0, 0, 0], 1)
    assert list(st) == [_lib.FIT_EXACT, _lib.FIT_EXACT, _lib.FIT_PRUNED, _lib.FIT_EXACT]
    exact = np.array([1.0, 1.0, 2.0, 1.0])
    vals = stored(st, exact, np.array(lower))
    assert select_best(records(vals, [1, 1, 1, 1])) == select_best(records(exact, [1, 1, 1, 1])) == (3, 1.0)


def test_degenerate_specials_and_empty_groups():
    # no converged candidate: all SKIPPED, no winner
    st = prune([0.1, 0.2], [0.3, 0.4], [0, 0], [0, 0], 3)
    assert list(st) == [_lib.FIT_SKIPPED] * 2
    # DBL_MAX / +inf: a DBL_MAX score can still win (<= the initial best), +inf never; lower +inf > upper DBL_MAX prunes
    st = prune([BIG, np.inf], [BIG, np.inf], [1, 1], [1, 1], 2)
    assert list(st) == [_lib.FIT_EXACT, _lib.FIT_PRUNED]
    vals = stored(st, np.array([BIG, np.inf]), np.array([BIG, np.inf]))
    assert select_best(records(vals, [1, 1])) == select_best(records(np.array([BIG, np.inf]), [1, 1])) == (0, BIG)
    # a NaN bound: the whole group exact
    st = prune([0.1, np.nan, 5.0], [0.2, 1.0, 6.0], [1, 1, 1], [0, 0, 0], 1)
    assert list(st) == [_lib.FIT_EXACT] * 3
    # group -1 next to grouped pairs: always exact, even when not converged and far above everything
    st = prune([9.0, 0.1, 9.0], [9.0, 0.2, 9.0], [0, 1, 1], [-1, 0, 0], 1)
    assert list(st) == [_lib.FIT_EXACT, _lib.FIT_EXACT, _lib.FIT_PRUNED]
    # no certified interval (0, +inf): never pruned, prunes nothing
    st = prune([0.0, 5.0], [np.inf, 6.0], [1, 1], [0, 0], 1)
    assert list(st) == [_lib.FIT_EXACT, _lib.FIT_EXACT]
    # zero pairs
    assert len(prune([], [], [], [], 0)) == 0


def test_cap_marks_only_lower_bounds_above_it():
    st = prune([0.5, 1.3, 1.25, 2.0], [np.inf, 1.4, 1.3, 2.5], [1, 1, 1, 1], [0, 0, 0, 0], 1, cap=1.25)
    assert list(st) == [_lib.FIT_EXACT, _lib.FIT_ABOVE_CAP, _lib.FIT_EXACT, _lib.FIT_PRUNED]


def test_invalid_groups_are_refused():
    L = _lib.lib()
    lo = np.zeros(2)
    cv = np.ones(2, dtype=np.int32)
    st = np.zeros(2, dtype=np.int32)
    for bad in ([0, 2], [-2, 0]):
        gr = np.array(bad, dtype=np.int32)
        rc = L.mrgfe_dbg_select_prune(2, lo.ctypes.data_as(_dp), lo.ctypes.data_as(_dp), cv.ctypes.data_as(_ip), gr.ctypes.data_as(_ip), 2, BIG, st.ctypes.data_as(_ip))
        assert rc == _lib.ERR_INVALID
