"""The serving path's graph captures run with the cyclic garbage collector
paused (``rtrec_amd.serving.retrieval._capture``): a collection that starts
inside a capture could finalise a dead index / searcher cycle, whose pinned
buffers and graphs cannot be freed while a stream is capturing. Checked without
a GPU, with a stand-in for ``torch.cuda.graph``."""
import contextlib
import gc
import weakref

import pytest
import torch


class _Node:
    pass


def _dead_cycle():
    a, b = _Node(), _Node()
    a.other, b.other = b, a
    return weakref.ref(a)


@pytest.fixture
def fake_graph(monkeypatch):
    seen = {}

    @contextlib.contextmanager
    def graph(g, capture_error_mode=None):
        seen["mode"] = capture_error_mode
        seen["gc_enabled_inside"] = gc.isenabled()
        yield
    monkeypatch.setattr(torch.cuda, "graph", graph)
    return seen


def test_no_collection_starts_inside_a_capture(fake_graph):
    from rtrec_amd.serving.retrieval import _capture
    assert gc.isenabled()
    old = gc.get_threshold()
    gc.set_threshold(1, 1, 1)   # any container allocation would start a collection
    try:
        # the control: outside a capture the allocations below do collect such a cycle
        dead = _dead_cycle()
        junk = [[] for _ in range(1000)]
        assert dead() is None
        with _capture(object()):
            dead = _dead_cycle()
            junk = [[] for _ in range(1000)]
            assert not gc.isenabled() and dead() is not None
        assert gc.isenabled() and fake_graph == {"mode": "thread_local", "gc_enabled_inside": False}
        del junk
        gc.collect()                      # the cycle was collectable all along
        assert dead() is None
    finally:
        gc.set_threshold(*old)


def test_capture_restores_the_collector_state(fake_graph):
    from rtrec_amd.serving.retrieval import _capture
    with pytest.raises(RuntimeError):
        with _capture(object()):
            raise RuntimeError("capture body failed")
    assert gc.isenabled()
    gc.disable()
    try:
        with _capture(object()):
            pass
        assert not gc.isenabled()   # it was off before: it stays off
    finally:
        gc.enable()


def test_both_serving_captures_go_through_it():
    import inspect
    from rtrec_amd.serving import online, retrieval
    assert "with _capture(g):" in inspect.getsource(retrieval.OnlineSearcher.search)
    assert "with _capture(g):" in inspect.getsource(online.OnlineRecommender._run)
