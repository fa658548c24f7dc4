"""Offline evaluation THROUGH an index (generate_recommendations(...,
index_config=...) and the CLI's --index-type): a small seeded model over
synthetic tables, 2,048 items and 64 users, "IVF32,Flat". With every list
probed the index's (scores, ids) are the exact call's, bit for bit; with nprobe
= 4 every user's list is the Flat oracle's search restricted to the lists that
user probes (tests/_ivf_ref.py), train items excluded."""
import json

import numpy as np
import pytest
import torch

import _ivf_ref as ref

pytestmark = pytest.mark.gpu

N_ITEMS, N_USERS, D, FU, FI, NLIST, TOP_K = 2048, 64, 32, 5, 7, 32, 100


@pytest.fixture(scope="module")
def world():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from rtrec_amd import native
    from rtrec_amd.models.two_tower import ItemTower, TwoTowerModel, UserTower
    native.lib()
    torch.manual_seed(0)
    model = TwoTowerModel(UserTower(FU, embedding_dim=D, hidden_layers=[32, 16], dropout_rate=0.2),
                          ItemTower(FI, embedding_dim=D, hidden_layers=[32, 16], use_content_embedding=False)).cuda()
    model.eval()
    rng = np.random.default_rng(1)
    uf = rng.standard_normal((N_USERS, FU)).astype(np.float32)
    mf = rng.standard_normal((N_ITEMS, FI)).astype(np.float32)
    train = {u: sorted(rng.choice(N_ITEMS, int(rng.integers(0, 300)), replace=False).tolist()) for u in range(N_USERS)}
    train[3] = []                                   # a user without train items
    users = rng.permutation(N_USERS).tolist()       # rows of the result are not user order
    return model, uf, mf, train, users


def _cfg(nprobe):
    return {"index_type": "hip_ivf", "index_factory": f"IVF{NLIST},Flat", "nprobe": nprobe}


def _host(pair):
    torch.cuda.synchronize()
    return pair[0].cpu().numpy(), pair[1].cpu().numpy()


def test_every_list_probed_is_the_exact_evaluation(world):
    from rtrec_amd.evaluation import generate_recommendations
    model, uf, mf, train, users = world
    es, ei = _host(generate_recommendations(model, users, train, uf, mf, top_k=TOP_K, return_tensors=True))
    info = {}
    gs, gi = _host(generate_recommendations(model, users, train, uf, mf, top_k=TOP_K, return_tensors=True,
                                            index_config=_cfg(NLIST), index_info=info))
    assert np.array_equal(gi, ei)
    assert np.array_equal(gs.view(np.uint32), es.view(np.uint32))
    assert info == {"index_type": "hip_ivf", "nlist": NLIST, "nprobe": NLIST}
    # the dict form goes through the same lists
    recs = generate_recommendations(model, users, train, uf, mf, top_k=TOP_K, index_config=_cfg(NLIST))
    assert recs == {u: [int(x) for x in ei[r] if x >= 0] for r, u in enumerate(users)}
    with pytest.raises(ValueError, match="1..128"):   # the index's own error
        generate_recommendations(model, users, train, uf, mf, top_k=129, index_config=_cfg(NLIST))


def test_nprobe_4_is_the_search_restricted_to_the_probed_lists(world):
    from rtrec_amd.evaluation import generate_recommendations
    from rtrec_amd.evaluation.offline import build_eval_index
    model, uf, mf, train, users = world
    nprobe = 4
    gs, gi = _host(generate_recommendations(model, users, train, uf, mf, top_k=TOP_K, return_tensors=True,
                                            index_config=_cfg(nprobe)))
    dev = torch.device("cuda")
    with torch.no_grad():
        item_emb = model.get_item_embeddings({"numerical": torch.from_numpy(mf).to(dev), "categorical": {}})
        user_emb = model.get_user_embeddings({"numerical": torch.from_numpy(uf[users]).to(dev), "categorical": {}})
    index = build_eval_index(item_emb.contiguous(), _cfg(nprobe))   # the build is deterministic: the same lists
    assert index.batch_min_queries == 1 and index.metric == "inner_product" and index._flat is None
    assign = index.assign.cpu().numpy()
    q = np.ascontiguousarray(user_emb.float().cpu().numpy())
    x = np.ascontiguousarray(item_emb.float().cpu().numpy())
    probes = ref.coarse_probes(q, index.centroids.cpu().numpy(), nprobe)
    mask = np.zeros((N_USERS, N_ITEMS), bool)
    for r, u in enumerate(users):
        mask[r, train[u]] = True
    rs, ri = ref.probed_lists_search(q, x, assign, probes, TOP_K, exclude_bits=ref.bitmap_of_excluded(mask))
    for r, u in enumerate(users):
        ids = gi[r][gi[r] >= 0]
        assert not set(ids.tolist()) & set(train[u]), "a train item was recommended"
        assert np.isin(assign[ids], probes[r]).all(), "an item outside the probed lists"
    assert np.array_equal(gi, ri)
    assert np.array_equal(gs.view(np.uint32), rs.view(np.uint32))


def test_cli_writes_the_retrieval_block(world, tmp_path):
    """--index-type hip_ivf --synthetic with nprobe = nlist: the block names the
    index and its recall@k against the exact lists is 1.0 for every k."""
    from rtrec_amd import evaluate_model as em
    from rtrec_amd.training.utils import create_two_tower_model_for_training
    torch.manual_seed(5)
    m = create_two_tower_model_for_training(3, 20, {"embedding_dim": 32, "hidden_layers": [32, 16]})
    ckpt = tmp_path / "two_tower_best.pth"
    torch.save({"user_tower_state": m.user_tower.state_dict(), "item_tower_state": m.item_tower.state_dict(),
                "temperature": 0.1}, ckpt)
    base = ["--synthetic", "--checkpoint", str(ckpt), "--k-values", "5,10,100"]
    res = em.run(em.build_parser().parse_args(base + ["--output", str(tmp_path / "ivf.json"), "--index-type", "hip_ivf",
                                                      "--index-factory", "IVF32,Flat", "--nprobe", "32"]))
    r = json.loads((tmp_path / "ivf.json").read_text())
    assert r["retrieval"] == {"index_type": "hip_ivf", "nlist": 32, "nprobe": 32,
                              "recall@5": 1.0, "recall@10": 1.0, "recall@100": 1.0}
    assert r["num_test_users"] > 1000 and 0.0 <= r["recall@10"] <= 1.0 and "diversity@10" in r
    assert all(len(v) == 100 for v in res["recommendations"].values())
    # the parser's default is the exact evaluation: no index, no block
    assert em.index_config_from_args(em.build_parser().parse_args(base)) is None
