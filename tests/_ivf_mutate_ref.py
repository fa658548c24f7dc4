"""Numpy model of IVF lists stored with slack (include/rtrec_hip.h,
rt_ivf_lists_update) for the mutation tests: the list state and its invariants,
the update semantics, the placement rule, and the renumbering rule of
HipMutableIVFFlatIndex.remove. Nothing here touches a GPU.

State: list l owns the stored rows [offsets[l], offsets[l + 1]); its live rows
are the first list_len[l]; row_pos is -1 behind them; pos_slot / assign map a
position to its stored row / list (-1: none)."""
import numpy as np


def capacities(lengths, list_slack=0.25, min_slack_rows=32):
    """len + max(min_slack_rows, ceil(len x list_slack)) per list."""
    lengths = np.asarray(lengths, np.int64)
    return lengths + np.maximum(min_slack_rows, np.ceil(lengths * list_slack).astype(np.int64))


class ListState:
    """The six state arrays. ``rows`` holds raw row bytes as uint8 [total, row_bytes]."""

    NAMES = ("rows", "list_len", "row_pos", "pos_slot", "assign")

    def __init__(self, caps, row_bytes):
        caps = np.asarray(caps, np.int64)
        self.offsets = np.concatenate([[0], np.cumsum(caps)]).astype(np.int64)
        self.nlist, self.total = len(caps), int(self.offsets[-1])
        self.rows = np.zeros((self.total, row_bytes), np.uint8)
        self.list_len = np.zeros(self.nlist, np.int64)
        self.row_pos = np.full(self.total, -1, np.int32)
        self.pos_slot = np.full(self.total, -1, np.int32)
        self.assign = np.full(self.total, -1, np.int64)

    def copy(self):
        c = ListState.__new__(ListState)
        c.offsets, c.nlist, c.total = self.offsets, self.nlist, self.total
        for name in self.NAMES:
            setattr(c, name, getattr(self, name).copy())
        return c

    def cap(self, l):
        return int(self.offsets[l + 1] - self.offsets[l])

    def fill(self, assignment, rows):
        """Positions 0 .. n - 1 with rows [n, row_bytes] into their lists, in position order."""
        for p, l in enumerate(np.asarray(assignment)):
            s = int(self.offsets[l] + self.list_len[l])
            assert self.list_len[l] < self.cap(l)
            self.rows[s], self.row_pos[s], self.pos_slot[p], self.assign[p] = rows[p], p, s, l
            self.list_len[l] += 1
        return self

    # -- the contract ------------------------------------------------------
    def apply(self, positions, new_list, new_rows):
        """rt_ivf_lists_update with the header's placement rule. Returns (overflowing
        lists, refused operations); the state changes only when both are 0."""
        positions, new_list = np.asarray(positions, np.int64), np.asarray(new_list, np.int64)
        assert len(set(positions.tolist())) == len(positions), "positions are unique: the caller's contract"
        refused = int(((positions < 0) | (positions >= self.total) | (new_list < -1) | (new_list >= self.nlist)).sum())
        if refused:
            return 0, refused
        old = self.assign[positions]
        old_slot = self.pos_slot[positions].copy()   # before any list writes: a mover's entry changes
        new_len = self.list_len.copy()
        for o, nl in zip(old, new_list):
            if o != nl:
                if o >= 0:
                    new_len[o] -= 1
                if nl >= 0:
                    new_len[nl] += 1
        over = int((new_len > np.diff(self.offsets)).sum())
        if over:
            return over, 0
        for l in range(self.nlist):
            off, ln = int(self.offsets[l]), int(self.list_len[l])
            stay = [i for i in range(len(positions)) if old[i] == l and new_list[i] == l]
            leave = [i for i in range(len(positions)) if old[i] == l and new_list[i] != l]
            join = [i for i in range(len(positions)) if old[i] != l and new_list[i] == l]   # ascending op order
            if not (stay or leave or join):
                continue
            for i in stay:
                self.rows[old_slot[i]] = new_rows[i]
            holes = sorted(int(old_slot[i]) - off for i in leave)   # ascending slot order
            for i in leave:
                self.row_pos[old_slot[i]] = -1
                if new_list[i] < 0:
                    self.pos_slot[positions[i]] = -1
                    self.assign[positions[i]] = -1
            n_new = ln - len(leave) + len(join)
            for j, i in enumerate(join):
                s = off + (holes[j] if j < len(holes) else ln + j - len(holes))
                self.rows[s], self.row_pos[s] = new_rows[i], positions[i]
                self.pos_slot[positions[i]], self.assign[positions[i]] = s, l
            spare = [h for h in holes[len(join):] if h < n_new]
            tail = [s for s in range(n_new, ln) if self.row_pos[off + s] >= 0]
            assert len(spare) == len(tail)
            for h, s in zip(spare, tail):
                p = self.row_pos[off + s]
                self.rows[off + h], self.row_pos[off + h], self.pos_slot[p] = self.rows[off + s], p, off + h
                self.row_pos[off + s] = -1
            self.list_len[l] = n_new
        return 0, 0

    def renumber(self, moves):
        """``moves`` {old position: new position} of remove's rule, applied to the state."""
        for p, t in moves.items():
            s = self.pos_slot[p]
            self.row_pos[s], self.pos_slot[t], self.assign[t] = t, s, self.assign[p]
            self.pos_slot[p], self.assign[p] = -1, -1


def check_invariants(st, offsets=None):
    """The invariants every call leaves, on a ListState or on anything with the same
    attributes (device arrays copied to numpy)."""
    offsets = st.offsets if offsets is None else offsets
    total = int(offsets[-1])
    row_pos, pos_slot, assign, list_len = (np.asarray(getattr(st, n)) for n in ("row_pos", "pos_slot", "assign",
                                                                                "list_len"))
    assert len(row_pos) == len(pos_slot) == len(assign) == total
    for l in range(len(offsets) - 1):
        off, cap, ln = int(offsets[l]), int(offsets[l + 1] - offsets[l]), int(list_len[l])
        assert 0 <= ln <= cap, (l, ln, cap)
        live = row_pos[off:off + ln]
        assert (live >= 0).all() and (live < total).all(), (l, live)
        assert (row_pos[off + ln:off + cap] == -1).all(), (l, row_pos[off + ln:off + cap])
        assert (assign[live] == l).all(), l
        assert np.array_equal(pos_slot[live], np.arange(off, off + ln)), l
    has = np.nonzero(pos_slot >= 0)[0]
    assert len(has) == int(list_len.sum())
    assert np.array_equal(row_pos[pos_slot[has]], has)          # the two maps name each other
    assert ((assign >= 0) == (pos_slot >= 0)).all()


def facts(st):
    """{position: (row bytes, list)} — what a state holds, whatever the placement."""
    pos_slot, assign, rows = np.asarray(st.pos_slot), np.asarray(st.assign), np.asarray(st.rows)
    return {int(p): (rows[pos_slot[p]].tobytes(), int(assign[p])) for p in np.nonzero(pos_slot >= 0)[0]}


def renumber_moves(n, removed):
    """remove's rule: with R = ``removed`` and n' = n - |R|, the surviving positions
    >= n' take, in ascending order, the removed positions < n', in ascending order.
    Returns ({old: new}, n')."""
    gone = set(int(p) for p in removed)
    n_new = n - len(gone)
    targets = sorted(p for p in gone if p < n_new)
    movers = [p for p in range(n_new, n) if p not in gone]
    assert len(targets) == len(movers)
    return dict(zip(movers, targets)), n_new


def renumber_moves_sequential(n, removed):
    """The same rule, one step at a time: the index shrinks from its end by one
    position per step; a removed last position just drops off, a surviving one
    moves into the highest remaining hole. A hole is a removed position that is
    still inside the index when all steps are done (< n'): a removed position
    further up drops off the end itself, and filling it first would move an item
    twice and may pair the items differently (n = 5, R = {0, 1, 2}: the rule
    gives 3 -> 0 and 4 -> 1; through the hole at 2 it would be 4 -> 2 -> 0 and
    3 -> 1)."""
    gone = set(int(p) for p in removed)
    n_new = n - len(gone)
    holes = sorted(p for p in gone if p < n_new)
    moves, last = {}, n - 1
    while last >= n_new:
        if last not in gone:
            moves[last] = holes.pop()
        last -= 1
    assert not holes
    return moves, n_new


class IndexModel:
    """Item-level model of HipMutableIVFFlatIndex: per position an id, a row (any
    hashable / array payload) and a list; update / add / remove as documented."""

    def __init__(self, ids, rows, lists):
        self.ids, self.rows, self.lists = list(ids), [r for r in rows], [int(l) for l in lists]

    def where(self):
        """id -> position of its LAST row (reverse_id_map)."""
        return {i: p for p, i in enumerate(self.ids)}

    def update(self, ids, rows, lists):
        last = {i: j for j, i in enumerate(ids)}          # the last occurrence wins
        where = self.where()
        fresh = []
        for i, j in last.items():
            if i in where:
                self.rows[where[i]], self.lists[where[i]] = rows[j], int(lists[j])
            else:
                fresh.append(j)
        self.add([ids[j] for j in fresh], [rows[j] for j in fresh], [lists[j] for j in fresh])

    def add(self, ids, rows, lists):
        self.ids += list(ids)
        self.rows += [r for r in rows]
        self.lists += [int(l) for l in lists]

    def remove(self, ids):
        hit = set(ids)
        removed = [p for p, i in enumerate(self.ids) if i in hit]
        moves, n_new = renumber_moves(len(self.ids), removed)
        for p, t in moves.items():
            self.ids[t], self.rows[t], self.lists[t] = self.ids[p], self.rows[p], self.lists[p]
        del self.ids[n_new:], self.rows[n_new:], self.lists[n_new:]
        return len(removed), moves
