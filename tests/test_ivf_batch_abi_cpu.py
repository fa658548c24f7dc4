"""C-ABI checks of the list-major IVF batch search (csrc/ivf_batch.hip) that
need no GPU: the three symbols are exported and in the ctypes table, every
refusal comes back as the documented status before any device work (the
pointers are dummies), the host-only plan keeps its invariants over a sweep,
its bound of the work items holds for seeded random and adversarial probe
tables counted in numpy, and the plan header (csrc/ivf_batch_plan.h) gives the
same numbers as a stand-alone program built with g++ under ASan + UBSan and run
as a child process: nothing preloaded, nothing loaded into Python."""
import ctypes
import itertools
import subprocess

import numpy as np
import pytest

from conftest import PKG, REPO

SYMBOLS = ["rt_ivf_topk_batch", "rt_ivf_topk_batch_plan", "rt_ivf_topk_batch_workspace_bytes",
           "rt_ivf_topk_batch_tuning"]
OK, INVALID, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3
F32, F16, BF16 = 0, 1, 2
TILE, MAX_LISTS = 128, 512

SWEEP = [(nq, nprobe, nlist, mlr, k)
         for nq, nprobe, nlist, mlr, k in itertools.product(
             (1, 31, 32, 33, 300, 4096, 100000), (1, 3, 20, 128), (1, 16, 1024, 65536),
             (0, 1, 127, 128, 129, 700, 1024, 1025, 5000, 300000), (1, 100, 128))]


@pytest.fixture(scope="module")
def native():
    from rtrec_amd import native as nat
    if not (PKG / "lib" / "librtrec_hip.so").exists():
        subprocess.run(["make", "-s", "-j8", "-C", str(PKG)], check=True)
    nat.lib()
    return nat


def _plan(L, nq, nprobe, nlist, mlr, k):
    out = (ctypes.c_int64 * 5)()
    rc = L.rt_ivf_topk_batch_plan(nq, nprobe, nlist, mlr, k, ctypes.cast(out, ctypes.c_void_p))
    return rc, tuple(out)


def test_symbols_exported_and_callable(native):
    handle = native.lib()
    for name in SYMBOLS:
        assert hasattr(handle, name), name
        assert name in native.SIGNATURES, name
    assert not native.MISSING
    rc, (qt, rpc, chunks, bound, blocks) = _plan(handle, 4096, 20, 1024, 2500, 100)
    assert rc == OK and qt == 32 and rpc % TILE == 0 and chunks * rpc >= 2500 and blocks >= 1
    assert handle.rt_ivf_topk_batch_workspace_bytes(4096, 20, 1024, 2500, 100) >= 4096 * 100 * 20 * chunks * 8
    assert handle.rt_ivf_topk_batch(None, 0, None, 0, 32, F32, None, 16, None, 0, None, None, 4, 0, 10, None, 0,
                                    None, None, None, 0, None) == OK   # nq == 0: nothing is read


P16 = ctypes.c_void_p(64)   # a non-NULL, 16-byte aligned dummy: never dereferenced by a refusal


def _batch(L, **kw):
    a = dict(queries=P16, nq=40, rows=P16, nx=1000, d=32, dtype=F32, offsets=P16, nlist=16, list_len=None, n_pos=0,
             row_pos=P16, probes=P16, nprobe=4, max_list_rows=300, k=10, excl=None, words=0, out_s=P16, out_i=P16,
             ws=P16, ws_bytes=0)
    a.update(kw)
    return L.rt_ivf_topk_batch(a["queries"], a["nq"], a["rows"], a["nx"], a["d"], a["dtype"], a["offsets"],
                               a["nlist"], a["list_len"], a["n_pos"], a["row_pos"], a["probes"], a["nprobe"],
                               a["max_list_rows"], a["k"], a["excl"], a["words"], a["out_s"], a["out_i"], a["ws"],
                               a["ws_bytes"], None)


def test_refusals_before_device_work(native):
    L = native.lib()
    for name in ("queries", "rows", "offsets", "row_pos", "probes", "out_s", "out_i"):
        assert _batch(L, **{name: None}) == INVALID, name
    assert _batch(L, k=0) == INVALID
    assert _batch(L, k=-3) == INVALID
    assert _batch(L, nprobe=0) == INVALID
    assert _batch(L, nlist=0) == INVALID
    assert _batch(L, nlist=-1) == INVALID
    assert _batch(L, nq=-1) == INVALID
    assert _batch(L, nx=-1) == INVALID
    assert _batch(L, max_list_rows=-1) == INVALID
    assert _batch(L, list_len=P16, n_pos=-1) == INVALID
    assert _batch(L, k=129) == UNSUPPORTED
    assert _batch(L, nprobe=129) == UNSUPPORTED
    assert _batch(L, dtype=3) == INVALID
    assert _batch(L, d=0) == INVALID
    assert _batch(L, d=260) == UNSUPPORTED            # d <= 256
    assert _batch(L, d=6) == UNSUPPORTED              # f32: d % 4
    assert _batch(L, d=12, dtype=F16) == UNSUPPORTED  # 16-bit: d % 8
    assert _batch(L, d=12, dtype=BF16) == UNSUPPORTED
    assert _batch(L, nx=2**31 - 1) == UNSUPPORTED
    assert _batch(L, list_len=P16, n_pos=2**31 - 1) == UNSUPPORTED
    assert _batch(L, nq=2**31 // 4) == UNSUPPORTED    # nq x nprobe >= 2^31
    assert _batch(L, queries=ctypes.c_void_p(72)) == INVALID   # misaligned
    assert _batch(L, rows=ctypes.c_void_p(72)) == INVALID
    assert _batch(L, excl=P16, words=31) == INVALID            # 1000 positions need 32 words
    assert _batch(L, list_len=P16, n_pos=2000, excl=P16, words=62) == INVALID   # n_pos, not nx, sizes the bitmap
    # everything valid but the workspace: NULL, one byte short, misaligned
    W = L.rt_ivf_topk_batch_workspace_bytes(40, 4, 16, 300, 10)
    assert W > 256 and W % 256 == 0
    assert _batch(L, ws=None, ws_bytes=W) == WORKSPACE
    assert _batch(L, ws_bytes=W - 1) == WORKSPACE
    assert _batch(L, ws=ctypes.c_void_p(68), ws_bytes=W) == INVALID
    assert _batch(L, nq=0) == OK
    with pytest.raises(native.RTError):
        native.call("rt_ivf_topk_batch", None, 1, None, 0, 32, 0, None, 1, None, 0, None, None, 1, 0, 1, None, 0,
                    None, None, None, 0, None)


def test_plan_refusals(native):
    L = native.lib()
    out = (ctypes.c_int64 * 5)()
    p = ctypes.cast(out, ctypes.c_void_p)
    assert L.rt_ivf_topk_batch_plan(1, 20, 16, 100, 10, None) == INVALID
    assert L.rt_ivf_topk_batch_plan(0, 20, 16, 100, 10, p) == INVALID
    assert L.rt_ivf_topk_batch_plan(1, 0, 16, 100, 10, p) == INVALID
    assert L.rt_ivf_topk_batch_plan(1, 20, 0, 100, 10, p) == INVALID
    assert L.rt_ivf_topk_batch_plan(1, 20, 16, -1, 10, p) == INVALID
    assert L.rt_ivf_topk_batch_plan(1, 20, 16, 100, 0, p) == INVALID
    assert L.rt_ivf_topk_batch_plan(1, 129, 16, 100, 10, p) == UNSUPPORTED
    assert L.rt_ivf_topk_batch_plan(1, 20, 16, 100, 129, p) == UNSUPPORTED
    assert L.rt_ivf_topk_batch_plan(2**31 // 20, 20, 16, 100, 10, p) == UNSUPPORTED
    assert L.rt_ivf_topk_batch_workspace_bytes(1, 129, 16, 100, 10) == 256
    assert L.rt_ivf_topk_batch_workspace_bytes(1, 20, 16, 100, 129) == 256
    assert L.rt_ivf_topk_batch_workspace_bytes(0, 20, 16, 100, 10) == 256
    # the measurement hook: a stage mask in [0, 7], 0 = the default
    assert L.rt_ivf_topk_batch_tuning(8) == INVALID and L.rt_ivf_topk_batch_tuning(-1) == INVALID
    assert L.rt_ivf_topk_batch_tuning(0) == OK


def _check_plan(nq, nprobe, nlist, mlr, k, plan, ws):
    qt, rpc, chunks, bound, blocks = plan
    pairs = nq * nprobe
    assert qt == 32
    assert rpc >= TILE and rpc % TILE == 0
    assert chunks >= 1 and chunks * rpc >= mlr
    assert (chunks - 1) * rpc < max(mlr, 1)                # no chunk past the longest list
    assert nprobe * chunks <= MAX_LISTS
    assert bound == (pairs // qt + min(nlist, pairs)) * chunks
    assert 1 <= blocks < 2**31 - 1 and blocks >= bound
    assert ws == -(-(8 * nq * k * nprobe * chunks + 4 * (3 * nlist + 2 + 2 * pairs)) // 256) * 256


def test_plan_invariants_and_workspace_formula(native):
    L = native.lib()
    planned = 0
    for nq, nprobe, nlist, mlr, k in SWEEP:
        rc, plan = _plan(L, nq, nprobe, nlist, mlr, k)
        ws = L.rt_ivf_topk_batch_workspace_bytes(nq, nprobe, nlist, mlr, k)
        if rc != OK:
            assert rc == UNSUPPORTED and ws == 256
            continue
        _check_plan(nq, nprobe, nlist, mlr, k, plan, ws)
        planned += 1
    assert planned > len(SWEEP) * 9 // 10
    # monotone in nq, every other argument fixed
    for nprobe, nlist, mlr, k in itertools.product((1, 20, 128), (16, 1024), (0, 700, 5000, 300000), (1, 100)):
        sizes = [L.rt_ivf_topk_batch_workspace_bytes(nq, nprobe, nlist, mlr, k)
                 for nq in (1, 2, 31, 32, 33, 64, 300, 4096, 4097, 100000)]
        assert sizes == sorted(sizes) and sizes[0] >= 256, (nprobe, nlist, mlr, k, sizes)


def _work_items(probes, nlist, qt, chunks):
    """(list, tile of qt pairs, chunk) items a probe table really has."""
    valid = probes[(probes >= 0) & (probes < nlist)]
    counts = np.bincount(valid, minlength=nlist)
    return int((-(-counts // qt)).sum()) * chunks


def test_work_items_stay_within_the_bound(native):
    L = native.lib()
    rng = np.random.default_rng(0)
    for nq, nprobe, nlist, mlr in [(1, 1, 16, 700), (33, 3, 16, 700), (300, 16, 16, 3000), (257, 20, 1024, 2500),
                                   (1000, 7, 50, 100), (64, 128, 128, 10)]:
        rc, (qt, rpc, chunks, bound, blocks) = _plan(L, nq, nprobe, nlist, mlr, 10)
        assert rc == OK
        tables = {
            "random": rng.integers(0, nlist, (nq, nprobe)),
            "skewed": np.minimum(rng.geometric(0.3, (nq, nprobe)) - 1, nlist - 1),
            "garbage": rng.integers(-3, nlist + 3, (nq, nprobe)),
            "one list": np.full((nq, nprobe), nlist - 1),
            "one list, one slot": np.concatenate([np.full((nq, 1), 2 % nlist), np.full((nq, nprobe - 1), -1)], axis=1),
            "all -1": np.full((nq, nprobe), -1),
        }
        if nq * nprobe <= nlist:   # every list probed exactly once (the rest of the table: none)
            flat = np.full(nq * nprobe, -1)
            flat[:] = rng.permutation(nlist)[:nq * nprobe]
            tables["each once"] = flat.reshape(nq, nprobe)
        else:                      # every list named, as evenly as the table allows
            tables["each list"] = (np.arange(nq * nprobe) % nlist).reshape(nq, nprobe)
        for name, t in tables.items():
            items = _work_items(np.asarray(t, np.int64), nlist, qt, chunks)
            assert items <= bound <= blocks, (name, nq, nprobe, nlist, items, bound)
        assert _work_items(np.asarray(tables["all -1"]), nlist, qt, chunks) == 0
    # every list probed exactly once: nlist items per chunk, the bound's min(nlist, P) term
    nlist = 64
    rc, (qt, rpc, chunks, bound, blocks) = _plan(L, 8, 8, nlist, 100, 10)
    each_once = rng.permutation(nlist).reshape(8, 8)
    assert _work_items(each_once, nlist, qt, chunks) == nlist * chunks <= bound


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("ivf_batch_plan") / "ivf_batch_plan_main"
    # the sanitizer runtimes linked statically: a dynamic ASan runtime refuses to
    # start when the environment preloads any other library ahead of it
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-I", str(PKG / "csrc"),
                    str(REPO / "tests" / "ivf_batch_plan_main.cpp"), "-o", str(exe)], check=True)
    return exe


def test_plan_header_stand_alone_under_sanitizers(native, plan_exe):
    """The same sweep through the header compiled with plain g++: no sanitizer
    report, the program's own invariant checks pass, and every line equals what
    the library answers."""
    L = native.lib()
    extra = [(2**31 // 20, 20, 16, 100, 10), (2**40, 1, 16, 100, 10), (1, 20, 2**31, 100, 10),
             (1, 20, 16, 2**32, 10), (100000, 128, 2**30, 2**31, 128)]
    grid = SWEEP + extra
    lines = []
    for a in range(0, len(grid), 500):   # argv stays short
        run = subprocess.run([str(plan_exe)] + [":".join(str(v) for v in g) for g in grid[a:a + 500]],
                             capture_output=True, text=True)
        assert run.returncode == 0, run.stderr[-4000:]
        assert not run.stderr, run.stderr[-4000:]  # a sanitizer report goes to stderr
        lines += run.stdout.split("\n")[:-1]
    assert len(lines) == len(grid)
    for g, ln in zip(grid, lines):
        got = tuple(int(x) for x in ln.split())
        rc, plan = _plan(L, *g)
        ws = L.rt_ivf_topk_batch_workspace_bytes(*g)
        if got[0] == 0:
            assert rc == UNSUPPORTED and ws == 256, g
        else:
            assert rc == OK and got[1:6] == plan and got[6] == ws, (g, got, plan, ws)
