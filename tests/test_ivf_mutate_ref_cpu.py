"""The numpy model of the mutable IVF lists (tests/_ivf_mutate_ref.py) against
itself: random update / add / remove sequences keep the invariants, hold exactly
the items a plain dictionary holds, and remove's renumbering rule equals its
sequential form. The GPU tests compare the kernel and the index with this
model, so it is checked here without one."""
import numpy as np
import pytest

import _ivf_mutate_ref as mref

NLIST, ROW_BYTES = 6, 16


def _row(rng):
    return rng.integers(0, 256, ROW_BYTES, dtype=np.uint8)


def _driver(seed, list_slack, min_slack_rows, steps=60):
    rng = np.random.default_rng(seed)
    n0 = 40
    assign0 = rng.integers(0, NLIST, n0)
    rows0 = np.stack([_row(rng) for _ in range(n0)])
    st = mref.ListState(mref.capacities(np.bincount(assign0, minlength=NLIST), list_slack, min_slack_rows), ROW_BYTES)
    st.fill(assign0, rows0)
    ids = [f"i{p}" for p in range(n0)]                      # position -> id
    truth = {ids[p]: (rows0[p].tobytes(), int(assign0[p])) for p in range(n0)}
    fresh = n0
    regroups = 0
    for step in range(steps):
        n = len(ids)
        kind = rng.choice(["update", "add", "remove"], p=[0.5, 0.25, 0.25])
        if kind == "remove" and n:
            removed = sorted(rng.choice(n, size=min(n, int(rng.integers(1, 6))), replace=False).tolist())
            moves, n_new = mref.renumber_moves(n, removed)
            assert (moves, n_new) == mref.renumber_moves_sequential(n, removed)
            assert st.apply(removed, [-1] * len(removed), np.zeros((len(removed), ROW_BYTES), np.uint8)) == (0, 0)
            st.renumber(moves)
            for p in removed:
                del truth[ids[p]]
            for p, t in moves.items():
                ids[t] = ids[p]
            del ids[n_new:]
        else:
            if kind == "update" and n:
                positions = rng.choice(n, size=min(n, int(rng.integers(1, 8))), replace=False).tolist()
            else:
                m = int(rng.integers(1, 8))
                positions = list(range(n, n + m))
                ids += [f"i{fresh + j}" for j in range(m)]
                fresh += m
            new_list = rng.integers(0, NLIST, len(positions))
            new_rows = np.stack([_row(rng) for _ in positions])
            status = (0, 0) if max(positions) < st.total else (1, 0)   # a position past the capacity: regroup
            if status == (0, 0):
                before = st.copy()
                status = st.apply(positions, new_list, new_rows)
                if status != (0, 0):   # all or nothing
                    for name in st.NAMES:
                        assert np.array_equal(getattr(st, name), getattr(before, name)), name
            if status != (0, 0):
                # the index's overflow path: one regroup of every live item, the batch included
                assert status[1] == 0
                regroups += 1
                have = mref.facts(st)
                for p, l, r in zip(positions, new_list, new_rows):
                    have[p] = (r.tobytes(), int(l))
                a = np.array([have[p][1] for p in range(len(ids))])
                st = mref.ListState(mref.capacities(np.bincount(a, minlength=NLIST), list_slack, min_slack_rows),
                                    ROW_BYTES)
                st.fill(a, np.stack([np.frombuffer(have[p][0], np.uint8) for p in range(len(ids))]))
            for p, l, r in zip(positions, new_list, new_rows):
                truth[ids[p]] = (r.tobytes(), int(l))
        mref.check_invariants(st)
        got = mref.facts(st)
        assert sorted(got) == list(range(len(ids))), step             # positions stay dense
        assert {ids[p]: v for p, v in got.items()} == truth, step
    return regroups


@pytest.mark.parametrize("seed", range(6))
def test_random_sequences_with_default_slack(seed):
    _driver(seed, 0.25, 32)


@pytest.mark.parametrize("seed", range(6))
def test_random_sequences_that_overflow(seed):
    """One spare row per list: batches overflow, nothing is written, the regroup holds the batch."""
    assert _driver(100 + seed, 0.0, 1) > 0


def test_capacity_rule():
    assert mref.capacities([0, 1, 100, 129, 1000]).tolist() == [32, 33, 132, 162, 1250]
    assert mref.capacities([0, 7], 0.0, 1).tolist() == [1, 8]


def test_renumbering_rule_by_hand():
    """n = 8, R = {1, 5, 6}: n' = 5, the survivor 7 takes 1; R = {0, 1, 4} of 6: 3 -> 0, 5 -> 1."""
    assert mref.renumber_moves(8, [1, 5, 6]) == ({7: 1}, 5)
    assert mref.renumber_moves(6, [0, 1, 4]) == ({3: 0, 5: 1}, 3)
    assert mref.renumber_moves(4, [0, 1, 2, 3]) == ({}, 0)
    rng = np.random.default_rng(7)
    for _ in range(200):
        n = int(rng.integers(1, 40))
        removed = rng.choice(n, size=int(rng.integers(1, n + 1)), replace=False).tolist()
        assert mref.renumber_moves(n, removed) == mref.renumber_moves_sequential(n, removed)


def test_placement_rule_by_hand():
    """One list of capacity 8 holding positions 0..5: positions 1 and 3 leave, 9 joins
    -> 9 takes slot 1 (the lowest hole), slot 3 takes the surviving tail row 5."""
    st = mref.ListState([8, 8], 16)
    rows = np.arange(6 * 16, dtype=np.uint8).reshape(6, 16)
    st.fill([0] * 6, rows)
    new = np.full((3, 16), 255, np.uint8)
    assert st.apply([1, 3, 9], [-1, 1, 0], new) == (0, 0)
    assert st.row_pos[:8].tolist() == [0, 9, 2, 5, 4, -1, -1, -1]
    assert st.row_pos[8:].tolist() == [3] + [-1] * 7
    assert st.list_len.tolist() == [5, 1]
    assert st.pos_slot[[0, 1, 2, 3, 4, 5, 9]].tolist() == [0, -1, 2, 8, 4, 3, 1]
    assert st.assign[[1, 3, 9]].tolist() == [-1, 1, 0]
    assert np.array_equal(st.rows[3], rows[5]) and np.array_equal(st.rows[1], new[2])
    mref.check_invariants(st)
    # overflow by one row: nothing changes
    before = st.copy()
    assert st.apply([10, 11, 12, 13], [0, 0, 0, 0], np.zeros((4, 16), np.uint8)) == (1, 0)
    assert st.apply([10], [2], np.zeros((1, 16), np.uint8)) == (0, 1)
    for name in st.NAMES:
        assert np.array_equal(getattr(st, name), getattr(before, name))
