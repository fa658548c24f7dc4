"""Beyond-accuracy list metrics without a GPU: the fp64 restatement the GPU
tests compare against equals the reference's own float64 values
(tests/golden/beyond_accuracy.npz, tools/make_goldens.py --only r4), the two
C entries validate every argument on the host and answer with rt_status
codes, and the public functions refuse CPU input instead of falling back."""
import ctypes
import gc
import subprocess

import numpy as np
import pytest
import torch

import _beyond_accuracy_ref as ref
from conftest import PKG, load_golden

INVALID, UNSUPPORTED = -1, -2


@pytest.fixture(scope="module", autouse=True)
def _collector_left_settled():
    """tests/test_capture_gc_cpu.py runs right after this module, and its control
    ("outside a capture these allocations do collect the cycle") holds only when
    the collector enters it with at least two young collections counted towards
    the middle generation: with fewer, its dead cycle is promoted to the oldest
    generation while still referenced and only a full collection would free it.
    The count it meets is whatever the preceding tests' allocations left, so
    this module leaves a known one: everything collected, then three young
    collections."""
    yield
    gc.collect()
    for _ in range(3):
        gc.collect(0)


@pytest.fixture(scope="module")
def native():
    from rtrec_amd import native as nat
    if not (PKG / "lib" / "librtrec_hip.so").exists():
        subprocess.run(["make", "-s", "-j8", "-C", str(PKG)], check=True)
    nat.lib()
    return nat


def test_restatement_equals_reference_float64():
    g = load_golden("beyond_accuracy")
    ks = [int(k) for k in g["k_values"]]
    assert ks == [2, 10, 100]
    lens = (g["lists"] >= 0).sum(axis=1)
    assert {0, 1, 2} <= set(lens.tolist()) and lens.max() == 100
    for name in ("table", "clustered"):
        assert g[name].dtype == np.float32 and g[name].shape == (300, 64)
        for i, k in enumerate(ks):
            got = ref.diversity(g["lists"], g[name], k)
            print(f"diversity {name} k={k}: restatement {got:.17g} reference f64 {g['div64_' + name][i]:.17g} "
                  f"(reference on fp32: {g['div32_' + name][i]:.17g})")
            assert abs(got - g["div64_" + name][i]) <= 1e-12
    for i, k in enumerate(ks):
        got = ref.novelty(g["lists"], g["pop_items"], g["pop_counts"], k)
        print(f"novelty k={k}: restatement {got:.17g} reference {g['novelty'][i]:.17g}")
        assert abs(got - g["novelty"][i]) <= 1e-12


def _ks(*v):
    return (ctypes.c_int32 * len(v))(*v)


def _list_args(**over):
    """A valid rt_list_metrics argument list over dummy pointers (no call that
    passes validation is made here: there is no device)."""
    p = ctypes.c_void_p(4096)
    a = dict(preds=p, n_rows=4, list_len=10, emb=p, dtype=0, n_emb=300, d=64, ld=64, info=p, n_info=300,
             default_info=1.0, k=_ks(2, 10), n_k=2, div=p, div_valid=p, nov_sum=p, nov_cnt=p, oob=None, stream=None)
    a.update(over)
    return [a[n] for n in ("preds", "n_rows", "list_len", "emb", "dtype", "n_emb", "d", "ld", "info", "n_info",
                           "default_info", "k", "n_k", "div", "div_valid", "nov_sum", "nov_cnt", "oob", "stream")]


def _reduce_args(**over):
    p = ctypes.c_void_p(4096)
    a = dict(div=p, div_valid=p, nov_sum=p, nov_cnt=p, n_rows=4, n_k=2, out=p, stream=None)
    a.update(over)
    return [a[n] for n in ("div", "div_valid", "nov_sum", "nov_cnt", "n_rows", "n_k", "out", "stream")]


_BAD_LIST = [
    ("preds NULL", dict(preds=None), INVALID),
    ("emb and info NULL", dict(emb=None, info=None), INVALID),
    ("div NULL", dict(div=None), INVALID),
    ("div_valid NULL", dict(div_valid=None), INVALID),
    ("nov_sum NULL", dict(nov_sum=None), INVALID),
    ("nov_cnt NULL", dict(nov_cnt=None), INVALID),
    ("k_values NULL", dict(k=None), INVALID),
    ("n_k 0", dict(n_k=0), INVALID),
    ("n_k 17", dict(k=_ks(*range(1, 18)), n_k=17), INVALID),
    ("k not ascending", dict(k=_ks(10, 10)), INVALID),
    ("k descending", dict(k=_ks(10, 2)), INVALID),
    ("k zero", dict(k=_ks(0, 2)), INVALID),
    ("d 0", dict(d=0, ld=0), INVALID),
    ("d 1028", dict(d=1028, ld=1028), UNSUPPORTED),
    ("fp16 d 20", dict(dtype=1, d=20, ld=20), UNSUPPORTED),
    ("bf16 d 20", dict(dtype=2, d=20, ld=20), UNSUPPORTED),
    ("row stride below d", dict(ld=32), INVALID),
    ("dtype 7", dict(dtype=7), INVALID),
    ("n_rows negative", dict(n_rows=-1), INVALID),
]

_BAD_REDUCE = [
    ("out NULL", dict(out=None), INVALID),
    ("all operands NULL", dict(div=None, div_valid=None, nov_sum=None, nov_cnt=None), INVALID),
    ("div without div_valid", dict(div_valid=None), INVALID),
    ("nov_sum without nov_cnt", dict(nov_cnt=None), INVALID),
    ("n_k 0", dict(n_k=0), INVALID),
    ("n_k 17", dict(n_k=17), INVALID),
    ("n_rows negative", dict(n_rows=-1), INVALID),
]


@pytest.mark.parametrize("what,over,status", _BAD_LIST, ids=[c[0] for c in _BAD_LIST])
def test_list_metrics_argument_errors(native, what, over, status):
    args = _list_args(**over)
    assert native.lib().rt_list_metrics(*args) == status, what
    with pytest.raises(native.RTError) as e:
        native.call("rt_list_metrics", *args)
    assert e.value.status == status


@pytest.mark.parametrize("what,over,status", _BAD_REDUCE, ids=[c[0] for c in _BAD_REDUCE])
def test_list_metrics_reduce_argument_errors(native, what, over, status):
    args = _reduce_args(**over)
    assert native.lib().rt_list_metrics_reduce(*args) == status, what
    with pytest.raises(native.RTError) as e:
        native.call("rt_list_metrics_reduce", *args)
    assert e.value.status == status


def test_no_rows_is_ok_without_a_device(native):
    assert native.lib().rt_list_metrics(*_list_args(n_rows=0)) == 0


def test_public_functions_refuse_cpu_input(native):
    from rtrec_amd.evaluation import compute_diversity, compute_novelty, list_metrics_tensors, self_information
    recs = {0: [1, 2, 3], 1: [4, 5]}
    emb = np.ones((8, 16), np.float32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        compute_diversity(recs, emb, k=2, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        compute_diversity(recs, torch.from_numpy(emb), k=2, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        compute_novelty(recs, {1: 3, 2: 5}, k=2, device="cpu")
    info, default = self_information({1: 3, 2: 5})
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        list_metrics_tensors(torch.tensor([[1, 2, -1]]), [2], item_info=info, default_info=default)


def test_self_information_table_and_contracts():
    """Host-side table: dict and count-tensor forms agree; a zero count in a
    tensor means absent (pop 1); an empty table with entries divides by zero
    as the reference does; negative ids are refused before any device work."""
    from rtrec_amd.evaluation import compute_diversity, compute_novelty, self_information
    info, default = self_information({0: 4, 2: 12})
    want = -np.log2(np.array([4, 1, 12]) / 16 + 1e-10)
    assert info.dtype == torch.float64 and np.array_equal(info.numpy(), want)
    assert default == float(-np.log2(1 / 16 + 1e-10))
    info_t, default_t = self_information(torch.tensor([4, 0, 12]))
    np.testing.assert_allclose(info_t.numpy(), want, rtol=0, atol=1e-14)
    assert default_t == default
    with pytest.raises(ZeroDivisionError):
        compute_novelty({0: [1, 2]}, {}, k=2, device="cpu")
    assert compute_novelty({0: []}, {}, k=2, device="cpu") == 0.0
    assert compute_diversity({}, np.ones((4, 8), np.float32), k=2, device="cpu") == 0.0
    with pytest.raises(ValueError):
        compute_diversity({0: [1, -2]}, np.ones((4, 8), np.float32), k=2, device="cpu")
