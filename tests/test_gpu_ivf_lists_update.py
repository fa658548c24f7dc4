"""rt_ivf_lists_update (csrc/ivf_mutate.hip) and the scan that reads list lengths
(rt_ivf_topk_lens, rt_ivf_topk_lists_lens) on hand-made lists with slack: nlist =
8, capacities 40-80 rows, d = 32 f32, then the narrowest row (d = 8 f16, 16
bytes) and the widest (d = 256 f32). The numpy model of tests/_ivf_mutate_ref.py
is the reference for the state — its invariants, what every position holds, and
(the placement rule being part of the header) every byte; the C oracle
restricted to the probed lists is the reference for the searches."""
import functools
import types

import numpy as np
import pytest
import torch

import _ivf_mutate_ref as mref
import _ivf_ref as ref

pytestmark = pytest.mark.gpu

F32, F16 = torch.float32, torch.float16
CASES = [(F32, 32), (F16, 8), (F32, 256)]
CASE_IDS = ["f32-d32", "f16-d8", "f32-d256"]
NLIST = 8
CAPS = [40, 48, 56, 64, 72, 80, 44, 60]
LENS = [30, 40, 20, 12, 0, 70, 30, 25]
N0 = sum(LENS)      # 227 positions at the start; positions up to sum(CAPS) - 1 = 463 are valid


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from rtrec_amd import kernels, native
    native.lib()
    return kernels


def _row_bytes(dt, d):
    return d * (4 if dt == F32 else 2)


def _rows(rng, n, dt, d):
    """n random rows as raw bytes uint8 [n, row_bytes] (finite values of ``dt``)."""
    t = torch.from_numpy(rng.standard_normal((n, d)).astype(np.float32)).to(dt).contiguous()
    return t.view(torch.uint8).numpy().reshape(n, _row_bytes(dt, d)).copy()


@functools.lru_cache(maxsize=None)
def _start(dt, d, caps=tuple(CAPS), lens=tuple(LENS)):
    """The state before any batch: positions 0 .. n0 - 1 dealt to the lists at random."""
    rng = np.random.default_rng(11 * d + (dt == F16))
    assign = rng.permutation(np.repeat(np.arange(NLIST), lens))
    st = mref.ListState(caps, _row_bytes(dt, d))
    st.fill(assign, _rows(rng, len(assign), dt, d))
    mref.check_invariants(st)
    return st


def _upload(st, dt):
    dev = types.SimpleNamespace(offsets=torch.from_numpy(st.offsets).cuda())
    for name in st.NAMES:
        setattr(dev, name, torch.from_numpy(getattr(st, name).copy()).cuda())
    dev.rows = dev.rows.view(dt)
    return dev


def _download(dev, st):
    torch.cuda.synchronize()
    got = types.SimpleNamespace(offsets=st.offsets)
    for name in st.NAMES:
        t = getattr(dev, name)
        got.__dict__[name] = (t.view(torch.uint8) if name == "rows" else t).cpu().numpy()
    return got


def _run(K, dev, positions, new_list, new_rows, dt):
    status = K.ivf_lists_update(dev.rows, dev.offsets, dev.list_len, dev.row_pos, dev.pos_slot, dev.assign,
                                torch.tensor(positions, dtype=torch.int64).cuda(),
                                torch.tensor(new_list, dtype=torch.int64).cuda(),
                                torch.from_numpy(new_rows).cuda().view(dt))
    return tuple(status.tolist())


def _assert_same(got, want, what):
    for name in mref.ListState.NAMES:
        assert np.array_equal(getattr(got, name), getattr(want, name)), (what, name)


def _check_batch(K, st, dt, positions, new_list, new_rows, what):
    """Apply one batch to the model and, twice from the same state, to the device."""
    want = st.copy()
    assert want.apply(positions, new_list, new_rows) == (0, 0), what
    mref.check_invariants(want)
    first = None
    for run in range(2):
        dev = _upload(st, dt)
        assert _run(K, dev, positions, new_list, new_rows, dt) == (0, 0), what
        got = _download(dev, st)
        mref.check_invariants(got)
        assert mref.facts(got) == mref.facts(want), what       # what every position holds, and its list
        _assert_same(got, want, what)                          # the placement rule: every byte
        if first is not None:
            _assert_same(got, first, what + ": second run")
        first = got
    return want


def _mixed_batch(st, dt, d):
    """One batch with, each in its own list: 0 leavers = joiners; 1 more leavers, three
    of them in the last slots; 2 more joiners; 3 emptied; 4 empty and joined; 5 filled
    exactly to capacity; 6 overwritten in place; 7 one of each."""
    rng = np.random.default_rng(5)

    def members(l, slots=None, count=None):
        live = st.row_pos[st.offsets[l]:st.offsets[l] + st.list_len[l]]
        if slots is None:
            slots = rng.choice(len(live), size=count, replace=False)
        return [int(live[s]) for s in slots]

    ops = []                                   # (position, new_list)
    fresh = iter(range(N0, N0 + 100))
    l0 = members(0, count=5)
    ops += [(p, 2) for p in l0[:2]] + [(p, -1) for p in l0[2:]]
    l1 = members(1, slots=[39, 38, 37, 3, 9, 17, 22, 30])
    ops += [(p, 2) for p in l1[:4]] + [(p, 5) for p in l1[4:6]] + [(p, -1) for p in l1[6:]]
    ops += [(next(fresh), 1) for _ in range(2)]
    ops += [(p, 4) for p in members(2, count=2)]
    ops += [(next(fresh), 2) for _ in range(4)]
    l3 = members(3, slots=range(12))
    ops += [(p, 0) for p in l3[:3]] + [(p, 4) for p in l3[3:8]] + [(p, 5) for p in l3[8:]]
    ops += [(next(fresh), 0) for _ in range(2)]
    ops += [(next(fresh), 5) for _ in range(4)]
    ops += [(p, 6) for p in members(6, count=6)]
    l7 = members(7, count=2)
    ops += [(l7[0], 7), (l7[1], -1), (next(fresh), 7)]
    order = rng.permutation(len(ops))          # operation order is not slot order
    positions = [ops[i][0] for i in order]
    new_list = [ops[i][1] for i in order]
    return positions, new_list, _rows(rng, len(ops), dt, d)


@pytest.mark.parametrize("dt,d", CASES, ids=CASE_IDS)
def test_mixed_batch_then_a_second(K, dt, d):
    st = _start(dt, d)
    positions, new_list, new_rows = _mixed_batch(st, dt, d)
    after = _check_batch(K, st, dt, positions, new_list, new_rows, "mixed")
    assert after.list_len.tolist() == [30, 34, 28, 0, 7, 80, 30, 25]
    assert after.list_len[5] == CAPS[5]                     # filled exactly
    # a second batch on the mutated state: the emptied list joined again, withdrawn positions reused
    rng = np.random.default_rng(6)
    gone = [p for p, l in zip(positions, new_list) if l == -1]
    back = [(p, 3) for p in gone] + [(int(p), 3) for p in after.row_pos[after.offsets[5]:after.offsets[5] + 20]]
    _check_batch(K, after, dt, [p for p, _ in back], [l for _, l in back], _rows(rng, len(back), dt, d), "second")


@pytest.mark.parametrize("dt,d", CASES, ids=CASE_IDS)
def test_300_operations_on_one_list(K, dt, d):
    """120 leavers, 60 overwrites and 120 joiners of one list in one batch: more
    operations than a workgroup has threads. The list is the one long list of a
    layout that is otherwise the small one."""
    caps, lens = list(CAPS), list(LENS)
    caps[1], lens[1] = 420, 200
    st = _start(dt, d, tuple(caps), tuple(lens))
    rng = np.random.default_rng(8)
    live = st.row_pos[st.offsets[1]:st.offsets[1] + 200]
    pick = rng.permutation(200)
    leavers, stayers = live[pick[:120]], live[pick[120:180]]
    n0 = sum(lens)
    ops = [(int(p), -1) for p in leavers[:100]] + [(int(p), 2) for p in leavers[100:]]
    ops += [(int(p), 1) for p in stayers] + [(n0 + j, 1) for j in range(120)]
    assert len(ops) == 300
    order = rng.permutation(300)
    _check_batch(K, st, dt, [ops[i][0] for i in order], [ops[i][1] for i in order], _rows(rng, 300, dt, d), "300")
    # and 220 joiners appended behind the 200 rows, no hole: the list filled exactly
    join = [(n0 + j, 1) for j in range(220)]
    after = _check_batch(K, st, dt, [p for p, _ in join], [1] * 220, _rows(rng, 220, dt, d), "append 220")
    assert after.list_len[1] == 420


@pytest.mark.parametrize("dt,d", CASES, ids=CASE_IDS)
def test_overflow_and_refusals_write_nothing(K, dt, d):
    st = _start(dt, d)
    rng = np.random.default_rng(9)
    stay = [int(p) for p in st.row_pos[st.offsets[6]:st.offsets[6] + 4]]      # would be overwritten
    move = [int(p) for p in st.row_pos[st.offsets[0]:st.offsets[0] + 3]]      # would move to list 2
    base = [(p, 6) for p in stay] + [(p, 2) for p in move]
    cases = {
        "overflow by one row": (base + [(N0 + j, 5) for j in range(11)], (1, 0)),     # 70 + 11 = cap + 1
        "new_list == nlist": (base + [(N0, NLIST)], (0, 1)),
        "new_list == -2": (base + [(N0, -2)], (0, 1)),
        "position == capacity": (base + [(sum(CAPS), 1)], (0, 1)),
        "position == -1": (base + [(-1, 1)], (0, 1)),
    }
    for what, (ops, want) in cases.items():
        dev = _upload(st, dt)
        got = _run(K, dev, [p for p, _ in ops], [l for _, l in ops], _rows(rng, len(ops), dt, d), dt)
        assert got == want, what
        _assert_same(_download(dev, st), st, what)        # every state buffer byte-identical
    model = st.copy()
    ops = cases["overflow by one row"][0]
    assert model.apply([p for p, _ in ops], [l for _, l in ops], _rows(rng, len(ops), dt, d)) == (1, 0)


def _bits(t):
    if t.dtype == F32:
        return t.numpy(), None
    return t.contiguous().view(torch.int16).numpy().view(np.uint16), 1


@pytest.mark.parametrize("dt,d", CASES, ids=CASE_IDS)
def test_scan_reads_lengths(K, dt, d):
    """On the mutated slack layout rt_ivf_topk_lens equals rt_ivf_topk on the same
    buffers (the -1 slots are dropped either way) and both equal the oracle over
    the rows in position order — without exclusions, with a bitmap of ceil(n_pos /
    32) words, and with exclusion lists (rt_ivf_topk_lists_lens)."""
    st = _start(dt, d).copy()
    positions, new_list, new_rows = _mixed_batch(st, dt, d)
    assert st.apply(positions, new_list, new_rows) == (0, 0)
    dev = _upload(st, dt)
    n_pos = int(np.nonzero(st.pos_slot >= 0)[0].max()) + 1
    assert n_pos < st.total and (st.pos_slot[:n_pos] < 0).any()      # withdrawn positions inside the range
    by_pos = np.zeros((n_pos, _row_bytes(dt, d)), np.uint8)
    has = st.pos_slot[:n_pos] >= 0
    by_pos[has] = st.rows[st.pos_slot[:n_pos][has]]
    x = torch.from_numpy(by_pos).view(dt)
    rng = np.random.default_rng(3)
    nq, k = 5, 10
    q = torch.from_numpy(rng.standard_normal((nq, d)).astype(np.float32)).to(dt)
    qa, code = _bits(q)
    xa = _bits(x)[0]
    mask = rng.random((nq, n_pos)) < 0.3
    bits = ref.bitmap_of_excluded(mask)
    assert bits.shape[1] == (n_pos + 31) // 32 < (st.total + 31) // 32
    wide = np.zeros((nq, (st.total + 31) // 32), np.uint32)          # rt_ivf_topk wants ceil(nx / 32) words
    wide[:, :bits.shape[1]] = bits
    lists = [np.nonzero(m)[0] for m in mask]
    lists[0] = np.concatenate([lists[0], [n_pos, n_pos + 7, st.total + 5]])       # items >= n_pos: ignored
    xo = np.zeros(nq + 1, np.int64)
    xo[1:] = np.cumsum([len(e) for e in lists])
    source = (torch.from_numpy(xo).cuda(), torch.from_numpy(np.concatenate(lists).astype(np.int32)).cuda())
    qd = q.cuda()
    max_cap = max(CAPS)
    for nprobe in (3, NLIST):
        probes = np.stack([rng.permutation(NLIST)[:nprobe] for _ in range(nq)]).astype(np.int64)
        pd = torch.from_numpy(probes).cuda()
        for what, want_bits in (("plain", None), ("excluded", bits)):
            rs, ri = ref.probed_lists_search(qa, xa, st.assign[:n_pos], probes, k, exclude_bits=want_bits,
                                             dtype_code=code)
            calls = {
                "lens": dict(list_len=dev.list_len, n_pos=n_pos,
                             exclude_bits=None if want_bits is None else torch.from_numpy(bits.view(np.int32)).cuda()),
                "no lens": dict(exclude_bits=None if want_bits is None
                                else torch.from_numpy(wide.view(np.int32)).cuda()),
            }
            if want_bits is not None:
                calls["lists lens"] = dict(list_len=dev.list_len, n_pos=n_pos, exclude_lists=[source])
            for name, kw in calls.items():
                gs, gi = K.ivf_topk(qd, dev.rows, dev.offsets, dev.row_pos, pd, max_cap, k, **kw)
                gs, gi = gs.cpu().numpy(), gi.cpu().numpy()
                assert np.array_equal(gi, ri), (nprobe, what, name)
                assert np.array_equal(gs.view(np.uint32), rs.view(np.uint32)), (nprobe, what, name)
    # a length below the live rows hides the rest: the scan reads list_len, not row_pos alone
    short = dev.list_len.clone()
    short[5] = 10
    probes = np.full((nq, 1), 5, np.int64)
    hidden = st.assign[:n_pos].copy()
    hidden[st.row_pos[st.offsets[5] + 10:st.offsets[5] + 80]] = -1
    rs, ri = ref.probed_lists_search(qa, xa, hidden, probes, k, dtype_code=code)
    gs, gi = K.ivf_topk(qd, dev.rows, dev.offsets, dev.row_pos, torch.from_numpy(probes).cuda(), max_cap, k,
                        list_len=short, n_pos=n_pos)
    assert np.array_equal(gi.cpu().numpy(), ri) and np.array_equal(gs.cpu().numpy().view(np.uint32), rs.view(np.uint32))
