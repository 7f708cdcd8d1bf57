"""Sharded dataset inference without a GPU: testing.ShardPlan over a sweep of sizes (every scene dealt once, local numbering contiguous,
the ranks' batches regrouped = the one-device batch list, empty ranks), the NumPy restatement of u3d_det_store_merge
(tests/det_merge_ref.py) against plain concatenation in dataset order and its refusals, the header / export / binding triple and the
argument checks of the new entry (answered before any launch, so they run here), and test_dataset's batch_ids on stub objects."""
import ctypes as C

import numpy as np
import pytest

import det_merge_ref as mref
import det_store_ref as ref
from test_abi_cpu import _Host
from test_det_store_cpu import _Step, _Store
from uni3detr_amd import abi
from uni3detr_amd import native as nv
from uni3detr_amd import testing
from uni3detr_amd.testing import ShardPlan

P, I, L = C.c_void_p, C.c_int32, C.c_int64
OK, ARG, UNSUPPORTED, WORKSPACE = 0, -1, -2, -4


# ---- the plan -------------------------------------------------------------------------------------------------------------------------
SWEEP = [(n, B, W) for n in (1, 5, 8, 9, 17) for B in (1, 2, 4) for W in (1, 2, 3, 8)]


@pytest.mark.parametrize("n, B, W", SWEEP)
def test_shard_plan(n, B, W):
    plan = ShardPlan(n, B, W)
    one_device = [list(range(j * B, min((j + 1) * B, n))) for j in range(-(-n // B))]
    m = plan.scene_map()
    assert m.dtype == np.int32 and m.shape == (n, 2)
    assert len({tuple(e) for e in m.tolist()}) == n                          # every (shard, local scene) exactly once
    regrouped = {}
    for r in range(W):
        order, ids = plan.order(r), plan.batch_ids(r)
        assert plan.scenes(r) == len(order)
        assert sorted(m[m[:, 0] == r, 1].tolist()) == list(range(plan.scenes(r)))          # locals contiguous from 0
        assert [m[p].tolist() for p in order] == [[r, k] for k in range(len(order))]        # ... in the order the rank runs them
        local = [order[k:k + B] for k in range(0, len(order), B)]            # what BatchFeeder(drop_last=False) makes of the order
        assert len(local) == len(ids) and ids == sorted(ids)
        assert all(len(b) == B for b in local[:-1])                           # only a rank's last batch can be partial
        for j, b in zip(ids, local):
            assert j % W == r and j // W == ids.index(j) and j not in regrouped
            regrouped[j] = b
        if not ids:
            assert plan.scenes(r) == 0 and order == []                       # an empty rank is legal
    assert [regrouped[j] for j in sorted(regrouped)] == one_device           # = the one-device batch list, exactly
    assert sum(plan.scenes(r) for r in range(W)) == n


def test_shard_plan_sweep_has_empty_ranks_and_takes_an_order():
    assert any(not ShardPlan(n, B, W).batch_ids(W - 1) for n, B, W in SWEEP)
    assert any(ShardPlan(n, B, W).scenes(0) % B for n, B, W in SWEEP if W > 1)             # a partial batch on a rank of several
    plan = ShardPlan(5, 2, 2)
    names = ["e", "d", "c", "b", "a"]
    assert plan.order(0, names) == ["e", "d", "a"] and plan.order(1, names) == ["c", "b"]
    assert plan.batch_ids(0) == [0, 2] and plan.batch_ids(1) == [1]
    assert ShardPlan(0, 2, 2).scene_map().shape == (0, 2)
    with pytest.raises(ValueError, match="rank 2"):
        plan.order(2)
    with pytest.raises(ValueError, match="4 entries"):
        plan.order(0, names[:4])
    with pytest.raises(ValueError, match="world"):
        ShardPlan(5, 2, 0)


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def _scene_list(det, n):
    b, s, l, c = det
    return [(b[i, :c[i]], s[i, :c[i]], l[i, :c[i]]) for i in range(n)]


def _sharded(rng, n, B, W, K, D):
    """-> (the W RefStores of a plan's ranks, the per-scene lists in dataset order): global batch j is random_det seeded by j"""
    plan = ShardPlan(n, B, W)
    stores = [ref.RefStore(max(plan.scenes(r), 1), max(plan.scenes(r), 1) * K, D, 0) for r in range(W)]
    whole = []
    for j in range(plan.n_batches):
        live = min((j + 1) * B, n) - j * B
        det = ref.random_det(np.random.default_rng(1000 + j), B, K, D, counts=rng.integers(0, K + 1, B))
        assert stores[j % W].append(*det, n_live=live)
        whole += _scene_list(det, live)
    return plan, stores, whole


@pytest.mark.parametrize("D", [7, 9])
@pytest.mark.parametrize("n, B, W", [(9, 2, 2), (4, 2, 3), (17, 4, 3), (5, 1, 8)])
def test_restatement_is_concatenation_in_dataset_order(n, B, W, D):
    plan, stores, whole = _sharded(np.random.default_rng(n + W), n, B, W, 5, D)
    got = mref.merged(stores, plan.scene_map()).pack()
    for name, g, w in zip(("boxes", "scores", "labels", "off"), got, ref.concat_lists(whole, D)):
        assert g.dtype == w.dtype and np.array_equal(g, w), name


def test_restatement_appends_behind_what_the_store_holds_and_copies_twice():
    rng = np.random.default_rng(3)
    plan, stores, whole = _sharded(rng, 5, 2, 2, 4, 7)
    early = ref.random_det(rng, 2, 4, 7, counts=[3, 1])
    dst = ref.RefStore(12, 80, 7, 0)
    assert dst.append(*early)
    m = np.concatenate([plan.scene_map(), plan.scene_map()[1:3]])             # scenes 1 and 2 named a second time
    assert mref.merge(dst, *mref.wire(stores), m)
    want = _scene_list(early, 2) + whole + whole[1:3]
    for g, w in zip(dst.pack(), ref.concat_lists(want, 7)):
        assert np.array_equal(g, w)
    assert dst.cursor.tolist() == [9, sum(w[1].shape[0] for w in want), 0, 0]
    assert np.isnan(dst.boxes[dst.cursor[1]:]).all() and (dst.table[9:] == ref.POISON_I).all()


def test_restatement_reads_offsets_clamped_and_refuses_whole_calls():
    rng = np.random.default_rng(4)
    plan, stores, _ = _sharded(rng, 6, 2, 2, 4, 7)
    w = mref.wire(stores, pad_f=np.nan, pad_i=ref.POISON_I)
    m = plan.scene_map()
    rows0 = int(w[4][0, 1])
    off = w[3].copy()
    off[0, 1], off[0, 3] = -5, rows0 + 9                                      # below 0 and past the shard's rows: read as 0 and as rows0
    dst = ref.RefStore(6, 60, 7, 0)
    assert mref.merge(dst, w[0], w[1], w[2], off, w[4], m)
    assert int(dst.cursor[1]) <= 60 and not np.isnan(dst.boxes[:dst.cursor[1]]).any()      # no padding row came along
    assert dst.table[0].tolist() == [0, 0]

    def refused(S=6, R=60, head=None, scene_map=m, cursor=None):
        d = ref.RefStore(S, R, 7, 0)
        if cursor:
            d.cursor[:2] = cursor
        before = {k: v.copy() for k, v in d.arrays().items()}
        ok = mref.merge(d, w[0], w[1], w[2], w[3], w[4] if head is None else head, scene_map)
        same = all(np.array_equal(before[k], v, equal_nan=True) for k, v in d.arrays().items() if k != "cursor")
        return (not ok) and same and d.cursor.tolist() == before["cursor"][:3].tolist() + [1]

    total = int(w[4][:, 1].sum())
    assert not refused() and not refused(R=total) and refused(R=total - 1) and refused(S=5)
    bad_shard, bad_local = m.copy(), m.copy()
    bad_shard[2, 0], bad_local[5, 1] = 2, int(w[4][m[5, 0], 0])
    assert refused(scene_map=bad_shard) and refused(scene_map=bad_local)
    bad_shard[2, 0] = -1
    assert refused(scene_map=bad_shard)
    for k, v in ((0, w[3].shape[1]), (1, w[0].shape[1] + 1), (1, -1)):
        head = w[4].copy()
        head[1, k] = v
        assert refused(head=head), (k, v)
    assert refused(cursor=(7, 0)) and refused(cursor=(0, -1)) and refused(cursor=(1, 0))   # outside the store; 1 + 6 scenes into 6


# ---- the ABI --------------------------------------------------------------------------------------------------------------------------
def test_entry_is_declared_exported_and_bound():
    protos = abi.load().prototypes
    assert protos["u3d_det_store_merge"] == (I, [P] * 5 + [I] * 4 + [P, I] + [P] * 6 + [I] * 3 + [P, L, P])
    assert protos["u3d_det_store_merge_workspace"] == (L, [I])
    raw = C.CDLL(nv.LIB_PATH)
    for name in ("u3d_det_store_merge", "u3d_det_store_merge_workspace"):
        assert name in nv.exported_symbols() and hasattr(raw, name)
        fn = getattr(nv.lib(), name)
        assert fn.restype is protos[name][0] and list(fn.argtypes) == protos[name][1]
    assert callable(nv.det_store_merge)
    assert nv.det_store_merge_workspace(0) > 0 and nv.det_store_merge_workspace(-3) == nv.det_store_merge_workspace(0)
    assert nv.det_store_merge_workspace(6019) - nv.det_store_merge_workspace(6018) <= 16    # linear in the scenes, a few words each


def test_merge_return_codes():
    h = _Host(16)

    def call(W=2, Nmax=10, Smax=3, D=7, n=4, R=64, S=8, M=0, null=None, invalid=False, ws=None):
        a = [None if null == k else h[k] for k in range(6)]                 # sh_boxes sh_scores sh_labels sh_off sh_head | scene_map
        st = [None if null == 6 + k else h[6 + k] for k in range(5)]        # store boxes scores labels table cursor
        work = None if null == 11 else h[12]
        ws = nv.det_store_merge_workspace(n) if ws is None else ws
        return nv.lib().u3d_det_store_merge(*a[:5], W, Nmax, Smax, D, a[5], n, *st, h[11] if invalid else None, R, S, M, work, ws, None)

    for k in range(12):
        assert call(null=k) == ARG, k
    assert call(W=0) == ARG and call(Nmax=0) == ARG and call(R=0) == ARG and call(S=0) == ARG and call(D=8) == ARG
    assert call(n=-1) == ARG and call(Smax=-1) == ARG and call(M=-1) == ARG
    assert call(M=2) == ARG and call(M=2, invalid=True, ws=0) == WORKSPACE   # M > 0 needs the list, as in append
    assert call(R=(2 ** 31) // 7 + 1) == UNSUPPORTED and call(D=9, R=(2 ** 31) // 9 + 1) == UNSUPPORTED
    assert call(W=4, Nmax=(2 ** 31) // 28 + 1) == UNSUPPORTED and call(W=4, Nmax=(2 ** 31) // 28 - 1, ws=0) == WORKSPACE
    assert call(D=8, R=2 ** 30) == ARG                                      # argument checks come before shape checks ...
    assert call(R=2 ** 30, ws=0) == UNSUPPORTED                             # ... and shape checks before the workspace's
    assert call(ws=nv.det_store_merge_workspace(4) - 1) == WORKSPACE and call(n=0, ws=nv.det_store_merge_workspace(0) - 1) == WORKSPACE


# ---- test_dataset(batch_ids=) on stubs ----------------------------------------------------------------------------------------------
def test_loop_hands_global_batch_ids_to_on_batch_and_reload():
    log = []
    step, store = _Step(log), _Store(log, invalid=[(2, 2), (4, 1)])
    ids = ShardPlan(11, 2, 2).batch_ids(1)                                   # rank 1 of two: global batches 1, 3, 5 (the last partial)
    assert ids == [1, 3, 5]
    reloaded = {3: ["r3a", "r3b"], 5: ["r5"]}

    def reload(j):
        log.append(("reload", j))
        return reloaded[j]

    batches = [["a", "b"], ["c", "d"], ["e"]]
    testing.test_dataset(step, batches, store, reload=reload, on_batch=lambda j: log.append(("on_batch", j)), batch_ids=ids)
    assert [e[1] for e in log if e[0] == "on_batch"] == [1, 3, 5, 3, 5]      # the loop, then the two repairs
    assert [e[1] for e in log if e[0] == "reload"] == [3, 5]
    assert [e for e in log if e[0] == "put"] == [("put", 2, ("eager-det", ["r3a", "r3b"])), ("put", 4, ("eager-det", ["r5"]))]
    # the default: the loop's own count, as before
    log.clear()
    testing.test_dataset(_Step(log), batches, _Store(log, invalid=[(2, 2)]), reload=lambda i: log.append(("reload", i)) or ["x", "y"],
                         on_batch=lambda i: log.append(("on_batch", i)))
    assert [e[1] for e in log if e[0] == "on_batch"] == [0, 1, 2, 1] and [e[1] for e in log if e[0] == "reload"] == [1]
    # the messages name the global batch
    with pytest.raises(RuntimeError, match="batch 3 .*no reload"):
        testing.test_dataset(_Step(log), batches, _Store(log, invalid=[(2, 2)]), batch_ids=ids)
    with pytest.raises(RuntimeError, match=r"reload\(3\) returned 1 scenes, batch 3 had 2"):
        testing.test_dataset(_Step(log), batches, _Store(log, invalid=[(2, 2)]), reload=lambda j: ["x"], batch_ids=ids)
