"""HipIVFFlatIndex with ``wide_k: True`` (k up to 1,024 through rt_ivf_topk_wide) on
the clustered 8,192 x 32 corpus of tests/_ivf_ref.py with "IVF64,Flat". Expected
ids and score bits are the C oracle's over the index's own prepared rows,
centroids and assignments (_ivf_ref.ivf_search / probed_lists_search)."""
import numpy as np
import pytest
import torch

import _ivf_ref as ref
from oracle import flat_ip as orc

pytestmark = pytest.mark.gpu
NLIST, D, NQ = 64, 32, 16
storages = pytest.mark.parametrize("storage", ["float32", "float16"])


@pytest.fixture(scope="module")
def R():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from rtrec_amd.serving import retrieval
    return retrieval


def _ids(n):
    return [f"item_{i}" for i in range(n)]


def _cfg(**kw):
    return {"dimension": D, "index_factory": f"IVF{NLIST},Flat", "metric": "cosine", "nprobe": 8, "wide_k": True, **kw}


_BUILT = {}


def _built(R, storage):
    """One wide index per storage dtype, shared and left unchanged."""
    if storage not in _BUILT:
        rows, _ = ref.clustered_corpus()
        idx = R.HipIVFFlatIndex(_cfg(storage_dtype=storage))
        idx.build(rows.copy(), _ids(len(rows)))
        _BUILT[storage] = idx
    return _BUILT[storage]


def _oracle_operands(idx):
    """(queries, rows, dtype_code, fp32 queries) as the oracle takes them: the index's own
    prepared queries and stored rows in original order, in its storage dtype."""
    q32 = idx._prepare(ref.clustered_corpus()[1][:NQ]).cpu()
    x = torch.from_numpy(idx.vectors())
    if idx.storage_dtype == torch.float32:
        return q32.numpy(), x.numpy(), None, q32.numpy()
    as_bits = lambda t: t.to(torch.float16).contiguous().view(torch.int16).numpy().view(np.uint16)
    return as_bits(q32), as_bits(x), 1, q32.numpy()


def _probed(idx, nprobe, k, exclude_bits=None):
    qa, xa, code, q32 = _oracle_operands(idx)
    probes = ref.coarse_probes(q32, idx.centroids.cpu().numpy(), nprobe)
    return ref.probed_lists_search(qa, xa, idx.assign.cpu().numpy(), probes, k, exclude_bits=exclude_bits,
                                   dtype_code=code)


def _equal(got, rs, ri):
    gs, gi = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert np.array_equal(gi, ri)
    assert np.array_equal(gs.view(np.uint32), rs.view(np.uint32))


@storages
def test_search_tensors(R, storage):
    """nprobe = nlist, k = 300: the Flat oracle's search; nprobe 8, k in {129, 1000}: the
    probed-lists search; k = 1025 raises and names 1..1024."""
    idx = _built(R, storage)
    queries = ref.clustered_corpus()[1][:NQ]
    qa, xa, code, _ = _oracle_operands(idx)
    _equal(idx.search_tensors(queries, 300, nprobe=NLIST), *orc.flat_ip_search(qa, xa, 300, dtype_code=code, nthreads=16))
    for k in (129, 1000):
        _equal(idx.search_tensors(queries, k), *_probed(idx, 8, k))
    with pytest.raises(ValueError, match=r"1\.\.1024"):
        idx.search_tensors(queries, 1025)


@storages
def test_search_with_exclude_and_filter_ids(R, storage):
    idx = _built(R, storage)
    queries, n, k = ref.clustered_corpus()[1][:NQ], 8192, 300
    _, plain = _probed(idx, 8, 2 * k)
    excl = [[f"item_{p}" for p in row[:7]] + ["unknown"] for row in plain]
    mask = np.zeros((NQ, n), bool)
    for i, row in enumerate(plain):
        mask[i, row[:7]] = True
    rs, ri = _probed(idx, 8, k, exclude_bits=ref.bitmap_of_excluded(mask))
    ids, scores = idx.search(queries, k, exclude_ids=excl)
    assert ids == [[f"item_{p}" for p in row if p >= 0] for row in ri]
    assert [np.float32(s) for s in scores[0]] == list(rs[0][ri[0] >= 0])
    allow = [f"item_{p}" for p in range(0, n, 3)]   # applied to the 2k over-fetch, in order, up to k
    ids, _ = idx.search(queries, k, filter_ids=allow)
    assert ids == [[f"item_{p}" for p in row if p >= 0 and p % 3 == 0][:k] for row in plain]


def test_engine_mutable_and_the_key(R, tmp_path):
    rows, queries = ref.clustered_corpus()
    eng = R.RetrievalEngine({"index_type": "hip_ivf", "embedding_dim": D, "top_k": 10,
                             "hip_ivf": {"index_factory": f"IVF{NLIST},Flat", "nprobe": 8, "wide_k": True}})
    eng.build_index(rows.copy(), _ids(len(rows)))
    ids, _, _ = eng.retrieve(queries[:2], k=200)
    assert [len(x) for x in ids] == [200, 200]
    # a mutable index after one update batch: at nprobe = nlist, a fresh build on the same rows
    changed = rows.copy()
    moved = np.arange(0, 400, 2)
    changed[moved] = rows[moved + 4000]
    mut = R.HipMutableIVFFlatIndex(_cfg())
    mut.build(rows.copy(), _ids(len(rows)))
    mut.update(changed[moved].copy(), [f"item_{p}" for p in moved])
    fresh = R.HipIVFFlatIndex(_cfg())
    fresh.build(changed, _ids(len(rows)))
    _equal(mut.search_tensors(queries[:NQ], 300, nprobe=NLIST),
           *(t.cpu().numpy() for t in fresh.search_tensors(queries[:NQ], 300, nprobe=NLIST)))
    # without the key: today's refusal; save / load keeps the key
    narrow = R.HipIVFFlatIndex({k: v for k, v in _cfg().items() if k != "wide_k"})
    narrow.build(rows.copy(), _ids(len(rows)))
    with pytest.raises(ValueError, match=r"returns 1\.\.128 results"):
        narrow.search_tensors(queries[:2], 129)
    wide = _built(R, "float32")
    wide.save(str(tmp_path / "idx"))
    other = R.HipIVFFlatIndex({"dimension": D, "nprobe": 8})   # nprobe is an attribute, not loaded
    assert not other.wide_k
    other.load(str(tmp_path / "idx"))
    assert other.wide_k
    _equal(other.search_tensors(queries[:NQ], 300), *(t.cpu().numpy() for t in wide.search_tensors(queries[:NQ], 300)))
