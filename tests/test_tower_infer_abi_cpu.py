"""rt_tower_infer_f32 at the C-ABI boundary, without a GPU: the ctypes mirrors
of rt_tower_layer / rt_tower_infer_args match the header (compiled here with
gcc), argument errors come back as rt_status codes before any launch (the
pointers are dummies), and OnlineRecommender refuses what it cannot serve."""
import ctypes
import subprocess

import pytest

from conftest import PKG, REPO

_LAYOUT_C = r"""
#include <stdio.h>
#include <stddef.h>
#include "rtrec_hip.h"
#define F(T, f) printf(#T " " #f " %zu\n", offsetof(T, f));
int main(void) {
  printf("rt_tower_layer size %zu\n", sizeof(rt_tower_layer));
  printf("rt_tower_infer_args size %zu\n", sizeof(rt_tower_infer_args));
  printf("max layers %d\n", RT_TOWER_MAX_LAYERS);
  printf("max rows %d\n", RT_TOWER_MAX_ROWS);
  printf("max width %d\n", RT_TOWER_MAX_WIDTH);
  %FIELDS%
  return 0;
}
"""


@pytest.fixture(scope="module")
def native():
    from rtrec_amd import native as nat
    if not (PKG / "lib" / "librtrec_hip.so").exists():
        subprocess.run(["make", "-s", "-j8", "-C", str(PKG)], check=True)
    nat.lib()
    return nat


def test_tower_struct_layout_matches_header(native, tmp_path):
    structs = (("rt_tower_layer", native.TowerLayer), ("rt_tower_infer_args", native.TowerInferArgs))
    lines = [f"F({cname}, {fname})" for cname, cls in structs for fname, _ in cls._fields_]
    src = tmp_path / "layout.c"
    src.write_text(_LAYOUT_C.replace("%FIELDS%", "\n  ".join(lines)))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", str(REPO / "include"), str(src), "-o", str(exe)], check=True)
    got = {}
    for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n"):
        if ln:
            t, f, v = ln.split()
            got[(t, f)] = int(v)
    for cname, cls in structs:
        assert got[(cname, "size")] == ctypes.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert got[(cname, fname)] == getattr(cls, fname).offset, (cname, fname)
    assert (got[("max", "layers")], got[("max", "rows")], got[("max", "width")]) == \
        (native.TOWER_MAX_LAYERS, native.TOWER_MAX_ROWS, native.TOWER_MAX_WIDTH) == (8, 8, 512)


def _args(native, widths=(10, 64, 32), m=1):
    """A well-formed argument set over fake non-NULL pointers (never launched)."""
    p16 = ctypes.c_void_p(16)
    a = native.TowerInferArgs()
    a.src, a.src_rows, a.ld_src, a.m, a.n_layers, a.normalize, a.out = p16, 8, widths[0], m, len(widths) - 1, 1, p16
    for i in range(len(widths) - 1):
        a.layers[i].w, a.layers[i].bias = p16, p16
        a.layers[i].k, a.layers[i].n = widths[i], widths[i + 1]
        a.layers[i].act = 0 if i < len(widths) - 2 else 5
    return a


def test_tower_argument_errors_are_status_codes(native):
    f = native.lib().rt_tower_infer_f32
    assert f(None, None) == -1
    for m in (0, 9):
        assert f(ctypes.byref(_args(native, m=m)), None) == -1, m
    for n_layers in (0, 9):
        a = _args(native)
        a.n_layers = n_layers
        assert f(ctypes.byref(a), None) == -1, n_layers
    assert f(ctypes.byref(_args(native, widths=(10, 513, 32))), None) == -2    # a width of 513
    assert f(ctypes.byref(_args(native, widths=(513, 64, 32))), None) == -2
    a = _args(native)
    a.layers[1].k = 48                                                          # != layers[0].n
    assert f(ctypes.byref(a), None) == -2
    a = _args(native)
    a.out = None
    assert f(ctypes.byref(a), None) == -1
    with pytest.raises(native.RTError):
        native.call("rt_tower_infer_f32", None, None)


def _cpu_model(**user_kw):
    from rtrec_amd.models.two_tower import ItemTower, TwoTowerModel, UserTower
    user = UserTower(10, embedding_dim=32, hidden_layers=[64], **user_kw)
    item = ItemTower(6, embedding_dim=32, hidden_layers=[64], use_content_embedding=False)
    return TwoTowerModel(user, item)


def test_recommender_refuses_a_cpu_model(native):
    from rtrec_amd.serving import HipFlatIPIndex, OnlineRecommender
    index = HipFlatIPIndex({"dimension": 32, "metric": "cosine"})
    with pytest.raises(RuntimeError, match="no CPU fallback") as ei:
        OnlineRecommender(_cpu_model(), index)
    assert isinstance(ei.value, ValueError)  # a refusal at construction, like the others


def test_recommender_refuses_categorical_towers_and_bad_shapes(native):
    from rtrec_amd.serving import HipFlatIPIndex, OnlineRecommender
    index = HipFlatIPIndex({"dimension": 32, "metric": "cosine"})
    with pytest.raises(ValueError, match="categorical"):
        OnlineRecommender(_cpu_model(categorical_features={"gender": 2}), index)
    with pytest.raises(ValueError, match="dimension"):
        OnlineRecommender(_cpu_model(), HipFlatIPIndex({"dimension": 64, "metric": "cosine"}))
    with pytest.raises(ValueError, match="inner-product"):
        OnlineRecommender(_cpu_model(), HipFlatIPIndex({"dimension": 32, "metric": "l2"}))
    from rtrec_amd.models.two_tower import UserTower
    with pytest.raises(ValueError, match="width"):
        OnlineRecommender(UserTower(10, embedding_dim=32, hidden_layers=[1024]), index)
    with pytest.raises(ValueError, match="Linear layers"):
        OnlineRecommender(UserTower(10, embedding_dim=32, hidden_layers=[16] * 8), index)
    with pytest.raises(ValueError):
        OnlineRecommender(_cpu_model(), index, max_batch=9)
